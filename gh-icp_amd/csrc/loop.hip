// GH-ICP iteration loop on gfx950: replaces GHRegistration::ghicp_reg and its private helpers
// (reference src/ghicp_reg.cpp:24-112, 114-139, 216-341, 343-460, 548-578, 605-927).
//
// Independent scan pairs are the parallel axis of this problem: the per-pair Kuhn-Munkres solve is one wave's dependency
// chain for most of its time, so throughput comes from many pairs in flight.  Every stage is a device function over a per-pair
// descriptor (LoopProb) in loop_dev.h, used in two ways:
//   * Kuhn-Munkres batches whose graphs fit the LDS-resident solver: the PERSISTENT pair loop k_pair_loop (pair_loop.hip) -- one 256-thread
//     workgroup is one solve slot, pops a pair from its class queue and runs the pair's whole ghicp_reg loop, iteration after iteration,
//     before it pops the next;
//   * NN / NNR batches and graphs beyond LDS: one launch per stage advances all pairs of the batch by one stage (the thin kernels of this
//     file around the same device functions); a pair that has converged makes its blocks exit at once, the host polls the `done` flags.
// Stages of one iteration (loop_dev.h; CD(i, j) itself is CdEval, the one place that spells it):
//   dev_cd_rowmin    fused calED + calCD_* + row arg-min (+ column arg-min sweep for NNR) + sum / sum^2 over
//                    K_S x K_T; no f64 ED/CD matrix is ever materialised                        (S5, HBM-bound)
//   dev_penalty      CDmean / CDstd -> penalty (calCD_* tails)                                    (scalar)
//   [KM] dev_km_row_count, dev_km_scan_desc, dev_km_row_fill (the sparse graph), then the exact Kuhn-Munkres solve: k4_solve_block
//        (km4_dev.h) inside the persistent loop, the launches of km4.hip / km.hip between the per-stage kernels      (S5 KM)
//   dev_solve        accept correspondences, RMSE/FDM/FDstd, float-Umeyama rigid solve, apply to all source
//                    keypoints, RMSE-after, Euler convergence test, adjustweight, Rt product       (S6)
// This file: the per-stage kernels, the hand-over of a batch, the arena and the host loop (run_loops), the C entry points.
#include "loop_dev.h"
int gh_km_solve_dev(ghicp_ctx* ctx, const double* w, int n, double eps, int32_t* match, const int* done_flag);

namespace {

template <int FT, bool COLS>
__global__ __launch_bounds__(ROWS) void k_cd_rowmin(const LoopProb* __restrict__ probs) {
  const LoopProb& P = probs[blockIdx.z];
  if (P.st->done) return;
  __shared__ double sB[CHUNK_MAX * 3];
  __shared__ double red[16];
  dev_cd_rowmin<FT, COLS>(P, (int)blockIdx.x, (int)blockIdx.y, sB, red);
}
__global__ __launch_bounds__(256) void k_penalty(const LoopProb* __restrict__ probs) {
  const LoopProb& P = probs[blockIdx.x];
  if (P.st->done) return;
  __shared__ double red[16];
  dev_penalty(P, red);
}

// Dense KM weights for the large-n fallback (ghicp_reg.cpp:348-365).
template <int FT>
__global__ __launch_bounds__(256) void k_km_weights(const LoopProb* __restrict__ probs) {
  const LoopProb& P = probs[blockIdx.z];
  if (P.st->done || P.kmw == nullptr) return;
  const LoopConst& C = P.C;
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int i = blockIdx.y;
  if (j >= C.n || i >= C.n) return;
  const double pen = P.st->penalty;
  double out = -pen;
  if (i < C.ks && j < C.kt) {
    const CdEval<FT> E(P, P.st->it);
    const double ed = E.ed(P.kpS[(size_t)i * 3], P.kpS[(size_t)i * 3 + 1], P.kpS[(size_t)i * 3 + 2], P.kpT[(size_t)j * 3], P.kpT[(size_t)j * 3 + 1], P.kpT[(size_t)j * 3 + 2]);
    const double cd = E.cd(ed, E.at(E.typed(P.FD), (size_t)i * C.kt + j));
    if (cd < pen) out = -cd;
  }
  P.kmw[(size_t)i * C.n + j] = out;
}
template <int FT, int FILL>
__global__ __launch_bounds__(256) void k_km_csr(const LoopProb* __restrict__ probs) {
  const LoopProb& P = probs[blockIdx.y];
  if (P.st->done || P.km_rptr == nullptr) return;
  dev_km_csr<FT, FILL>(P, (int)blockIdx.x);
}
__global__ __launch_bounds__(1024) void k_km_scan_desc(const LoopProb* __restrict__ probs) {
  const LoopProb& P = probs[blockIdx.x];
  if (P.st->done || P.km_rptr == nullptr) return;
  __shared__ int sc[17];
  dev_km_scan_desc(P, sc);
}
template <int FT>
__global__ __launch_bounds__(1024) void k_solve(const LoopProb* __restrict__ probs) {
  const LoopProb& P = probs[blockIdx.x];
  if (P.st->done) return;
  __shared__ double red[16];
  __shared__ int ired[17];
  __shared__ double sh[32];
  dev_solve<FT>(P, red, ired, sh);
}

// Hand-over of a batch in two launches instead of two per pair (5376 pairs a step: the per-pair copies, memsets and transposes were a
// launch-bound tail of every step, profiles/r03_kernel_stats_bench_default.txt): every pair's source keypoints into its own buffer ...
__global__ __launch_bounds__(256) void k_pairs_copy_kps(const LoopProb* __restrict__ probs, int pair0) {
  const LoopProb& P = probs[pair0 + blockIdx.y];
  const int n = P.C.ks * 3;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) P.kpS[i] = P.kpS_src[i];
}
// ... and every pair's feature-distance matrix transposed once so that the row sweep reads it coalesced (tiles beyond a pair's extent exit)
template <typename T> __global__ void k_pairs_transpose(const LoopProb* __restrict__ probs, int pair0) {
  const LoopProb& P = probs[pair0 + blockIdx.z];
  const int rows = P.C.ks, cols = P.C.kt;
  if (rows <= 0 || cols <= 0 || (int)blockIdx.x * 32 >= cols || (int)blockIdx.y * 32 >= rows || P.fdt_given) return;
  const T* __restrict__ in = reinterpret_cast<const T*>(P.FD);
  T* __restrict__ out = const_cast<T*>(reinterpret_cast<const T*>(P.FDt));
  __shared__ T tile[32][33];
  const int x = blockIdx.x * 32 + threadIdx.x, y0 = blockIdx.y * 32;
  for (int r = threadIdx.y; r < 32; r += blockDim.y)
    if (x < cols && y0 + r < rows) tile[r][threadIdx.x] = in[(size_t)(y0 + r) * cols + x];
  __syncthreads();
  const int ox = blockIdx.y * 32 + threadIdx.x, oy0 = blockIdx.x * 32;
  for (int r = threadIdx.y; r < 32; r += blockDim.y)
    if (ox < rows && oy0 + r < cols) out[(size_t)(oy0 + r) * rows + ox] = tile[threadIdx.x][r];
}
__global__ void k_collect_done(const LoopProb* __restrict__ probs, int n, int* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { out[i * 2] = probs[i].st->it; out[i * 2 + 1] = probs[i].st->done; }
}

static void pick_chunks(int ka, int kb, int batch, int* chunk, int* nchunk) {
  // aim for >= ~2048 workgroups per launch (256 CUs x 8) with chunks of at least 32 columns
  const int rowblocks = cdiv(ka > 0 ? ka : 1, ROWS) * (batch > 0 ? batch : 1);
  int want = cdiv(2048, rowblocks);
  int ch = cdiv(kb > 0 ? kb : 1, want);
  if (ch < 32) ch = 32;
  if (ch > CHUNK_MAX) ch = CHUNK_MAX;
  *chunk = ch;
  *nchunk = kb > 0 ? cdiv(kb, ch) : 1;
}

struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(char* b) : base(b) {}
  template <typename T> T* take(size_t count) {
    off = (off + 255) & ~(size_t)255;
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += count * sizeof(T);
    return p;
  }
};

// The batch's arena: the shared tables first, then every pair's buffers, each 256-byte aligned; and what the launches need to know of the batch
struct LoopLayout {
  size_t total;
  const double* wfd;
  LoopProb* dprobs;
  Km2Problem* d_descs;
  LoopState* dstates;
  int *dflags, *dqheads, *dkmst, max_rowsA, max_chunkB, max_rowsB, max_chunkA, max_n, max_ks, max_kt;
  bool need_transpose;
};
// Fills the pairs' descriptors hp[] and the layout; arena == nullptr: the size pass (total only, every pointer null)
template <int FT>
void layout_batch(char* arena, int nb, const gh_loop_job* jobs, size_t wtab_size, int chunk_batch, std::vector<LoopProb>& hp, LoopLayout& Y) {
  const int corr = jobs[0].p->corr;
  Carver cv(arena);
  Y.wfd = cv.take<double>(wtab_size);
  Y.dprobs = cv.take<LoopProb>(nb);
  Y.dflags = cv.take<int>((size_t)nb * 2);
  Y.dqheads = cv.take<int>(16);  // queue heads of the persistent pair loop, one per class
  Y.d_descs = cv.take<Km2Problem>(nb);  // contiguous: the dense-fallback path launches one solve kernel over all of them
  Y.dstates = cv.take<LoopState>(nb);   // contiguous states and solver status words: ONE upload / memset / download per batch
  Y.dkmst = cv.take<int>((size_t)nb + 1);
  Y.max_rowsA = Y.max_chunkB = Y.max_rowsB = Y.max_chunkA = Y.max_n = Y.max_ks = Y.max_kt = 1;
  Y.need_transpose = false;
  for (int b = 0; b < nb; b++) {
    const gh_loop_job& J = jobs[b];
    const ghicp_params* p = J.p;
    LoopProb& L = hp[b];
    memset(&L, 0, sizeof(L));
    LoopConst& C = L.C;
    const int ks = J.ks, kt = J.kt;
    C.ks = ks; C.kt = kt; C.n = ks > kt ? ks : kt; C.feature = p->feature; C.corr = p->corr; C.max_iter = p->max_iter; C.min_cor = p->min_cor;
    C.scale = (float)(0.005 * p->bbx_magnitude);  // ghicp_reg.h:40 (double product stored to float)
    C.est_iou = p->est_iou; C.adjust_ratio = p->adjust_ratio; C.adjust_step = p->adjust_step;
    C.converge_t = (double)p->converge_t; C.converge_r = (double)p->converge_r; C.penalty_initial = p->penalty_initial; C.km_eps = p->km_eps;
    pick_chunks(ks, kt, chunk_batch, &C.chunk_b, &C.nchunk_b);
    pick_chunks(kt, ks, chunk_batch, &C.chunk_a, &C.nchunk_a);
    C.nparts = cdiv(ks > 0 ? ks : 1, ROWS) * C.nchunk_b;
    Y.max_rowsA = std::max(Y.max_rowsA, cdiv(ks > 0 ? ks : 1, ROWS)); Y.max_chunkB = std::max(Y.max_chunkB, C.nchunk_b);
    Y.max_rowsB = std::max(Y.max_rowsB, cdiv(kt > 0 ? kt : 1, ROWS)); Y.max_chunkA = std::max(Y.max_chunkA, C.nchunk_a);
    Y.max_n = std::max(Y.max_n, C.n);
    L.wfd = Y.wfd;
    L.st = Y.dstates + b;
    L.kpS_src = J.kpS;
    Y.max_ks = std::max(Y.max_ks, ks); Y.max_kt = std::max(Y.max_kt, kt);
    L.kpS = cv.take<double>((size_t)ks * 3 + 3);
    L.kpT = J.kpT; L.FD = J.FD;
    L.pminA = cv.take<double>((size_t)C.nchunk_b * ks + 1);
    L.pidxA = cv.take<int>((size_t)C.nchunk_b * ks + 1);
    L.psum = cv.take<double>((size_t)C.nparts * 2 + 2);
    if (corr == GHICP_CORR_NNR) {
      L.pminB = cv.take<double>((size_t)C.nchunk_a * kt + 1);
      L.pidxB = cv.take<int>((size_t)C.nchunk_a * kt + 1);
    }
    L.SP = cv.take<int>((size_t)C.n + 1);
    L.TP = cv.take<int>((size_t)C.n + 1);
    L.SVs = cv.take<int>((size_t)ks + 1);
    L.TVs = cv.take<int>((size_t)kt + ks + 2);
    L.trace = cv.take<ghicp_iter>((size_t)p->max_iter + 1);
    L.matchlist = J.matchlist;
    L.ml_row0 = J.ml_row0;
    if (FT != GHICP_FEATURE_NONE) {
      if (J.FDt) L.FDt = J.FDt;  // the caller's batched feature-distance kernel wrote the transposed copy already
      else { L.FDt = cv.take<char>((size_t)ks * kt * (FT == GHICP_FEATURE_BSC ? 2 : 4) + 16); Y.need_transpose = true; }
      L.fdt_given = J.FDt != nullptr;
    }
    if (corr == GHICP_CORR_KM) {
      L.kmmatch = cv.take<int>((size_t)C.n + 1);
      L.km_status = Y.dkmst + b;
      if (gh_km4_fits(C.n)) {
        L.km_cnt = cv.take<unsigned>((size_t)C.n + 1);
        L.km_rptr = cv.take<unsigned>((size_t)C.n + 2);
        L.km_lx = cv.take<double>((size_t)C.n + 1);
        L.km_cols = cv.take<int>((size_t)ks * kt + 1);
        L.km_vals = cv.take<double>((size_t)ks * kt + 1);
        L.km_desc = Y.d_descs ? Y.d_descs + b : nullptr;
      } else {
        L.kmw = cv.take<double>((size_t)C.n * C.n + 1);
      }
    }
  }
  Y.total = cv.off;
}

// ---- upload tables, states, descriptors; the hand-over of the whole batch
template <int FT>
int upload_batch(ghicp_ctx* ctx, int nb, const gh_loop_job* jobs, const std::vector<double>& wtab, const std::vector<LoopProb>& hp,
                 std::vector<LoopState>& hst, const LoopLayout& Y) {
  hipStream_t s = ctx->stream;
  GH_HIP(hipMemcpyAsync(const_cast<double*>(Y.wfd), wtab.data(), wtab.size() * sizeof(double), hipMemcpyHostToDevice, s));
  GH_HIP(hipMemsetAsync(Y.d_descs, 0, (size_t)nb * sizeof(Km2Problem), s));  // n = 0: "nothing to solve"
  for (int b = 0; b < nb; b++) {
    LoopState& h = hst[b];
    memset(&h, 0, sizeof(h));
    h.RMS = 99999; h.para1 = jobs[b].p->para1; h.para2 = jobs[b].p->para2;  // ghicp_reg.h:98, 33-34
    for (int d = 0; d < 4; d++) h.Rt_till[d * 5] = 1.0;
    if (jobs[b].resume_in) {  // ghicp_iterate: the loop continues from the state the previous call left
      memcpy(&h, jobs[b].resume_in, sizeof(h));
      h.done = 0;
    }
    if (jobs[b].ks <= 0 || jobs[b].kt <= 0) h.done = 1;
  }
  GH_HIP(hipMemcpyAsync(Y.dstates, hst.data(), (size_t)nb * sizeof(LoopState), hipMemcpyHostToDevice, s));
  GH_HIP(hipMemsetAsync(Y.dkmst, 0, ((size_t)nb + 1) * sizeof(int), s));
  GH_HIP(hipMemcpyAsync(Y.dprobs, hp.data(), (size_t)nb * sizeof(LoopProb), hipMemcpyHostToDevice, s));
  // the hand-over of the whole batch: source keypoints into the pairs' own buffers, feature matrices transposed (k_pairs_*)
  for (int b0 = 0; b0 < nb; b0 += 65535)  // gridDim.y <= 65535
    hipLaunchKernelGGL(k_pairs_copy_kps, dim3(std::min(cdiv(Y.max_ks * 3, 256), 8), std::min(65535, nb - b0)), dim3(256), 0, s, (const LoopProb*)Y.dprobs, b0);
  if (FT != GHICP_FEATURE_NONE && Y.need_transpose) {
    const int tx = cdiv(Y.max_kt, 32), ty = cdiv(Y.max_ks, 32);
    const int zmax = (int)std::max<long long>(1, std::min<long long>(65535, (1ll << 22) / ((long long)tx * ty)));  // <= 4 M workgroups (2^30 threads) a launch
    for (int b0 = 0; b0 < nb; b0 += zmax) {
      const dim3 g(tx, ty, std::min(zmax, nb - b0));
      if (FT == GHICP_FEATURE_BSC) hipLaunchKernelGGL(k_pairs_transpose<uint16_t>, g, dim3(32, 8), 0, s, (const LoopProb*)Y.dprobs, b0);
      else hipLaunchKernelGGL(k_pairs_transpose<float>, g, dim3(32, 8), 0, s, (const LoopProb*)Y.dprobs, b0);
    }
  }
  GH_HIP(hipGetLastError());
  return GHICP_OK;
}

// ---- iterate, one launch per stage for all pairs of the batch; the host polls the `done` flags every other iteration
template <int FT>
int iterate_staged(ghicp_ctx* ctx, int nb, int max_iter, const std::vector<LoopProb>& hp, const LoopLayout& Y, bool any_sparse, bool any_dense,
                   int max_n_sparse, const Km4Plan* km_plan) {
  hipStream_t s = ctx->stream;
  const int corr = hp[0].C.corr;
  const LoopProb* dprobs = Y.dprobs;
  std::vector<int> hflags((size_t)nb * 2, 0);
  const int poll_every = 2;
  int launched = 0;
  bool all_done = false;
  while (!all_done && launched < max_iter) {
    for (int r = 0; r < poll_every && launched < max_iter; r++, launched++) {
      hipEvent_t kev = ctx->kt_begin(KT_CD_ROWMIN);
      hipLaunchKernelGGL((k_cd_rowmin<FT, false>), dim3(Y.max_rowsA, Y.max_chunkB, nb), dim3(ROWS), 0, s, dprobs);
      ctx->kt_end(KT_CD_ROWMIN, kev);
      if (corr == GHICP_CORR_NNR) hipLaunchKernelGGL((k_cd_rowmin<FT, true>), dim3(Y.max_rowsB, Y.max_chunkA, nb), dim3(ROWS), 0, s, dprobs);
      hipLaunchKernelGGL(k_penalty, dim3(nb), dim3(256), 0, s, dprobs);
      if (corr == GHICP_CORR_KM) {
        hipEvent_t kw = ctx->kt_begin(KT_KM_WEIGHTS);
        hipLaunchKernelGGL((k_km_csr<FT, 0>), dim3(cdiv(Y.max_n, 4), nb), dim3(256), 0, s, dprobs);
        hipLaunchKernelGGL(k_km_scan_desc, dim3(nb), dim3(1024), 0, s, dprobs);
        hipLaunchKernelGGL((k_km_csr<FT, 1>), dim3(cdiv(Y.max_n, 4), nb), dim3(256), 0, s, dprobs);
        ctx->kt_end(KT_KM_WEIGHTS, kw);
        if (any_sparse) GH_TRY(km_plan ? gh_km4_launch_plan(ctx, Y.d_descs, *km_plan) : gh_km4_launch(ctx, Y.d_descs, nb, max_n_sparse));
        if (any_dense) {  // matrices too large for the LDS-resident solver: dense fallback, one pair at a time
          hipLaunchKernelGGL(k_km_weights<FT>, dim3(cdiv(Y.max_n, 256), Y.max_n, nb), dim3(256), 0, s, dprobs);
          for (int b = 0; b < nb; b++)
            if (hp[b].kmw) GH_TRY(gh_km_solve_dev(ctx, hp[b].kmw, hp[b].C.n, hp[b].C.km_eps, hp[b].kmmatch, &hp[b].st->done));
        }
      }
      // 256 threads: four waves of this kernel (108 VGPRs) fit next to the Kuhn-Munkres waves of other batches on a CU;
      // a 1024-thread block needs a CU with no resident solve wave and stalls for a whole solve launch when batches overlap
      hipLaunchKernelGGL(k_solve<FT>, dim3(nb), dim3(256), 0, s, dprobs);
    }
    GH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_collect_done, dim3(cdiv(nb, 256)), dim3(256), 0, s, dprobs, nb, Y.dflags);
    GH_HIP(hipMemcpyAsync(hflags.data(), Y.dflags, hflags.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    GH_HIP(hipStreamSynchronize(s));
    all_done = true;
    long long still = 0;
    for (int b = 0; b < nb; b++) { all_done &= (hflags[(size_t)b * 2 + 1] != 0); still += hflags[(size_t)b * 2 + 1] == 0; }
    ctx->loop_active.store(still, std::memory_order_relaxed);
  }
  return GHICP_OK;
}

// ---- results and status
int download_results(ghicp_ctx* ctx, int nb, const gh_loop_job* jobs, const std::vector<LoopProb>& hp, std::vector<LoopState>& hst, const LoopLayout& Y,
                     bool persistent, bool any_dense) {
  hipStream_t s = ctx->stream;
  std::vector<int> hkmst((size_t)nb + 1, 0);
  GH_HIP(hipMemcpyAsync(hst.data(), Y.dstates, (size_t)nb * sizeof(LoopState), hipMemcpyDeviceToHost, s));
  GH_HIP(hipMemcpyAsync(hkmst.data(), Y.dkmst, ((size_t)nb + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
  GH_HIP(hipStreamSynchronize(s));
  if (ctx->kt_on && persistent) {  // slot timeline of the batch (diagnostics, ghicp_ctx_loop_timeline): per pair begin / end / iterations
    ctx->loop_timeline.resize((size_t)nb * 3);
    for (int b = 0; b < nb; b++) {
      // iterations [15:0] | iteration of the pair's longest solve [31:16] | that solve in units of 16 ticks = 160 ns [63:32]; where the slot
      // ran rides in the top bits of `begin` (ticks since boot need 48 bits): CU [55:52], shader array [56], engine [59:57], die [63:60]
      const unsigned hw = hst[b].hw_id;
      const unsigned long long where = (unsigned long long)((hw >> 8) & 0xFu) | ((unsigned long long)((hw >> 12) & 1u) << 4) | ((unsigned long long)((hw >> 13) & 7u) << 5) |
                                       ((unsigned long long)((hw >> 16) & 0xFu) << 8);
      ctx->loop_timeline[(size_t)b * 3] = (long long)((hst[b].t_begin & 0x000FFFFFFFFFFFFFull) | (where << 52));
      ctx->loop_timeline[(size_t)b * 3 + 1] = (long long)(hst[b].t_end & 0x000FFFFFFFFFFFFFull);
      ctx->loop_timeline[(size_t)b * 3 + 2] = (long long)(((unsigned long long)(hst[b].it & 0xFFFF)) | ((unsigned long long)(hst[b].it_solve_max & 0xFFFF) << 16) |
                                                          (std::min<unsigned long long>(hst[b].t_solve_max >> 4, 0xFFFFFFFFull) << 32));
    }
  }
  for (int b = 0; b < nb; b++) {
    const gh_loop_job& J = jobs[b];
    for (int d = 0; d < 16; d++) J.Rt16[d] = hst[b].Rt_till[d];
    if (J.n_iter) *J.n_iter = hst[b].it;
    if (J.converged) *J.converged = hst[b].converged_flag;
    if (J.rmse_after) *J.rmse_after = hst[b].rmse_after;
    if (J.trace && hst[b].it > 0) GH_HIP(hipMemcpyAsync(J.trace, hp[b].trace, (size_t)hst[b].it * sizeof(ghicp_iter), hipMemcpyDeviceToHost, s));
    if (J.trace_last && hst[b].it > 0) GH_HIP(hipMemcpyAsync(J.trace_last, hp[b].trace + (hst[b].it - 1), sizeof(ghicp_iter), hipMemcpyDeviceToHost, s));
    if (J.kpS_out && J.ks > 0) GH_HIP(hipMemcpyAsync(J.kpS_out, hp[b].kpS, (size_t)J.ks * 3 * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (J.resume_out) memcpy(J.resume_out, &hst[b], sizeof(LoopState));
  }
  GH_HIP(hipStreamSynchronize(s));
  int kmst = 0;
  for (int b = 0; b < nb; b++)
    if (hp[b].km_status) {
      kmst |= hkmst[(size_t)b] & 0xFFFF;
      ctx->loop_hazards += (long long)((unsigned)hkmst[(size_t)b] >> 16);  // solves through the literal fallback (diagnostics)
    }
  if (any_dense && ctx->buf[B_KM_MISC].p) {  // the dense fallback reports through the context's own status word
    int v = 0;
    GH_HIP(hipMemcpy(&v, ctx->buf[B_KM_MISC].p, sizeof(int), hipMemcpyDeviceToHost));
    kmst |= v;
  }
  if (kmst) return ctx->fail(GHICP_ERR_INTERNAL, "KM solver status %d (non-finite energy?)", kmst);
  return GHICP_OK;
}

template <int FT>
int run_loops(ghicp_ctx* ctx, int nb, const gh_loop_job* jobs) {
  // ghicp_ctx_set_loop_cost_hints: "consumed by the next registration call of this context, ignored otherwise" -- taken here, whatever
  // path the batch takes (round-4 advisor: cleared only in the Kuhn-Munkres branch, hints survived a batch of another kind)
  std::vector<float> cost_hints;
  cost_hints.swap(ctx->loop_cost_hints);
  const ghicp_params* p0 = jobs[0].p;
  const int corr = p0->corr;
  int max_iter = 1;
  for (int b = 0; b < nb; b++) max_iter = jobs[b].p->max_iter > max_iter ? jobs[b].p->max_iter : max_iter;
  // exp(-it/rate) from the host libm, exactly as calCD_BSC computes it (ghicp_reg.cpp:247); one table per batch
  std::vector<double> wtab(max_iter + 1);
  for (int i = 0; i <= max_iter; i++) wtab[i] = std::exp(-1.0 * i / p0->weight_changing_rate);

  std::vector<LoopProb> hp(nb);
  std::vector<LoopState> hst(nb);
  // Kuhn-Munkres batches whose every graph fits the LDS-resident solver run as the persistent pair loop (k_pair_loop)
  bool persistent = corr == GHICP_CORR_KM;
  for (int b = 0; b < nb && persistent; b++) {
    const int n = std::max(jobs[b].ks, jobs[b].kt);
    persistent = (jobs[b].ks <= 0 || jobs[b].kt <= 0) || gh_km4_fits(n);
  }
  const int chunk_batch = persistent ? (1 << 20) : nb;  // one workgroup sweeps a pair: the largest chunks (fewest partial sums)
  // ---- size pass, then carve every pair's buffers out of one allocation
  LoopLayout Y;
  layout_batch<FT>(nullptr, nb, jobs, wtab.size(), chunk_batch, hp, Y);
  char* arena = nullptr;
  GH_TRY(ctx->reserve(B_LOOP_STATE, Y.total + 4096, &arena));
  layout_batch<FT>(arena, nb, jobs, wtab.size(), chunk_batch, hp, Y);
  GH_TRY(upload_batch<FT>(ctx, nb, jobs, wtab, hp, hst, Y));

  // ---- iterate
  ctx->loop_total.store(nb, std::memory_order_relaxed);
  ctx->loop_active.store(nb, std::memory_order_relaxed);
  bool any_dense = false;
  for (int b = 0; b < nb; b++) any_dense |= (hp[b].kmw != nullptr);
  bool any_sparse = false;
  int max_n_sparse = 1;
  for (int b = 0; b < nb; b++)
    if (hp[b].km_rptr) { any_sparse = true; max_n_sparse = std::max(max_n_sparse, hp[b].C.n); }
  // the Kuhn-Munkres launches of this batch: problems grouped by LDS occupancy, largest first (km4.hip)
  Km4Plan km_plan;
  bool use_plan = false;
  if (any_sparse && !any_dense && gh_km4_fits(max_n_sparse)) {
    std::vector<int> hn((size_t)nb);
    bool all_sparse = true;
    for (int b = 0; b < nb; b++) { hn[b] = hp[b].C.n; all_sparse &= (hp[b].km_rptr != nullptr) || jobs[b].ks <= 0 || jobs[b].kt <= 0; }
    if (all_sparse) {
      // cost hints of the caller for exactly this batch (ghicp_ctx_set_loop_cost_hints): consumed once
      const bool hinted = (int)cost_hints.size() == nb;
      GH_TRY(gh_km4_plan(ctx, hn.data(), nb, &km_plan, hinted ? cost_hints.data() : nullptr));
      use_plan = true;
    }
  }
  if (persistent && use_plan) {
    const int rc = run_pair_loop<FT>(ctx, Y.dprobs, nb, km_plan, Y.dqheads);
    if (rc != GHICP_OK) {
      ctx->progress_live.store(false, std::memory_order_release);
      return rc;
    }
  } else {
    GH_TRY(iterate_staged<FT>(ctx, nb, max_iter, hp, Y, any_sparse, any_dense, max_n_sparse, use_plan ? &km_plan : nullptr));
  }
  ctx->loop_active.store(0, std::memory_order_relaxed);
  ctx->progress_live.store(false, std::memory_order_release);
  return download_results(ctx, nb, jobs, hp, hst, Y, persistent, any_dense);
}

}  // namespace

int gh_register_batch_dev(ghicp_ctx* ctx, int nb, const gh_loop_job* jobs) {
  if (nb <= 0) return GHICP_OK;
  for (int b = 0; b < nb; b++) {
    const gh_loop_job& J = jobs[b];
    GH_ARG(J.p != nullptr && J.Rt16 != nullptr);
    GH_ARG(J.ks >= 0 && J.kt >= 0 && J.p->max_iter > 0 && J.p->max_iter <= 100000);
    GH_ARG(J.p->corr == GHICP_CORR_NN || J.p->corr == GHICP_CORR_NNR || J.p->corr == GHICP_CORR_KM);
    GH_ARG(J.p->feature == jobs[0].p->feature && J.p->corr == jobs[0].p->corr && J.p->weight_changing_rate == jobs[0].p->weight_changing_rate);
    if (J.p->feature == GHICP_FEATURE_BSC || J.p->feature == GHICP_FEATURE_FPFH) GH_ARG(J.FD != nullptr || J.ks == 0 || J.kt == 0);
  }
  switch (jobs[0].p->feature) {
    case GHICP_FEATURE_BSC: return run_loops<GHICP_FEATURE_BSC>(ctx, nb, jobs);
    case GHICP_FEATURE_FPFH: return run_loops<GHICP_FEATURE_FPFH>(ctx, nb, jobs);
    case GHICP_FEATURE_NONE:
    case GHICP_FEATURE_ROPS:  // test/ghicp_main.cpp:130-134 falls through with no feature
      return run_loops<GHICP_FEATURE_NONE>(ctx, nb, jobs);
    default: return ctx->fail(GHICP_ERR_ARG, "unknown feature type %d", jobs[0].p->feature);
  }
}

int gh_register_dev(ghicp_ctx* ctx, const ghicp_params* p, const double* kpS, int ks, const double* kpT, int kt, const void* FD,
                    double* Rt16, ghicp_iter* trace, int32_t* n_iter, int32_t* matchlist) {
  gh_loop_job J;
  memset(&J, 0, sizeof(J));
  J.p = p; J.kpS = kpS; J.ks = ks; J.kpT = kpT; J.kt = kt; J.FD = FD; J.Rt16 = Rt16; J.trace = trace; J.n_iter = n_iter; J.matchlist = matchlist;
  return gh_register_batch_dev(ctx, 1, &J);
}

extern "C" int ghicp_register(ghicp_ctx* ctx, const ghicp_params* p, const double* kpS, int64_t ks, const double* kpT, int64_t kt,
                              const void* FD, double* Rt16, ghicp_iter* trace, int32_t* n_iter, int32_t* matchlist) {
  GH_ENTER(ctx);
  GH_ARG(p != nullptr && ks >= 0 && kt >= 0 && ks < (1 << 24) && kt < (1 << 24));
  Stager sg(ctx);
  const double *dS, *dT;
  GH_TRY(sg.in(kpS, (size_t)ks * 3, &dS));
  GH_TRY(sg.in(kpT, (size_t)kt * 3, &dT));
  const size_t esz = p->feature == GHICP_FEATURE_BSC ? 2 : 4;
  const char* dFD = nullptr;
  if (p->feature == GHICP_FEATURE_BSC || p->feature == GHICP_FEATURE_FPFH) GH_TRY(sg.in((const char*)FD, (size_t)ks * kt * esz, &dFD));
  int32_t* dml;
  GH_TRY(sg.out(matchlist, (size_t)p->max_iter * ks, &dml));
  GH_TRY(gh_register_dev(ctx, p, dS, (int)ks, dT, (int)kt, dFD, Rt16, trace, n_iter, dml));
  return sg.finish();
}

// ---- One step at a time (ghicp_iterate = one pass of calED ... adjustweight, src/ghicp_reg.cpp:49-103).  The state object owns
// the moving source keypoints and the scalar loop state (Rt_tillnow, RMS, FDM, FDstd, IoU, para1/2, iteration number) between calls; an
// iteration runs through the SAME batch path as ghicp_register (a batch of one pair, max_iter = it + 1), so a sequence of ghicp_iterate calls
// reproduces ghicp_register's trace bit for bit (tests/test_gpu_loop.py::test_iterate_equals_register).
struct ghicp_loop {
  ghicp_ctx* ctx;
  ghicp_params p;
  int ks, kt;
  DevBuf kpS, kpT, FD;  // own device copies: the caller's arrays may go away between two calls
  LoopState st;
  bool started, finished;
};

extern "C" int ghicp_loop_create(ghicp_ctx* ctx, const ghicp_params* p, const double* kpS, int64_t ks, const double* kpT, int64_t kt, const void* FD,
                                 ghicp_loop** out) {
  GH_ENTER(ctx);
  GH_ARG(p != nullptr && out != nullptr && ks >= 0 && kt >= 0 && ks < (1 << 24) && kt < (1 << 24));
  GH_ARG(p->corr == GHICP_CORR_NN || p->corr == GHICP_CORR_NNR || p->corr == GHICP_CORR_KM);
  const bool has_fd = p->feature == GHICP_FEATURE_BSC || p->feature == GHICP_FEATURE_FPFH;
  if (has_fd) GH_ARG(FD != nullptr || ks == 0 || kt == 0);
  *out = nullptr;
  ghicp_loop* L = new ghicp_loop();
  L->ctx = ctx; L->p = *p; L->ks = (int)ks; L->kt = (int)kt; L->started = false; L->finished = false;
  memset(&L->st, 0, sizeof(L->st));
  const hipMemcpyKind kind = ctx->host_ptrs ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  const size_t esz = p->feature == GHICP_FEATURE_BSC ? 2 : 4;
  hipError_t e = L->kpS.reserve((size_t)ks * 24 + 32);
  if (e == hipSuccess) e = L->kpT.reserve((size_t)kt * 24 + 32);
  if (e == hipSuccess && has_fd) e = L->FD.reserve((size_t)ks * kt * esz + 32);
  if (e == hipSuccess && ks > 0) e = hipMemcpyAsync(L->kpS.p, kpS, (size_t)ks * 24, kind, ctx->stream);
  if (e == hipSuccess && kt > 0) e = hipMemcpyAsync(L->kpT.p, kpT, (size_t)kt * 24, kind, ctx->stream);
  if (e == hipSuccess && has_fd && ks > 0 && kt > 0) e = hipMemcpyAsync(L->FD.p, FD, (size_t)ks * kt * esz, kind, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    L->kpS.release(); L->kpT.release(); L->FD.release();
    delete L;
    return ctx->fail(GHICP_ERR_HIP, "ghicp_loop_create: %s", hipGetErrorString(e));
  }
  *out = L;
  return GHICP_OK;
}

extern "C" int ghicp_iterate(ghicp_ctx* ctx, ghicp_loop* L, ghicp_iter* out, int32_t* match_row) {
  GH_ENTER(ctx);
  GH_ARG(L != nullptr && L->ctx == ctx && out != nullptr);
  if (L->finished) return ctx->fail(GHICP_ERR_ARG, "ghicp_iterate: the loop has converged (or has no keypoints); create a new one");
  ghicp_params p = L->p;
  p.max_iter = (L->started ? L->st.it : 0) + 1;  // exactly one more iteration
  Stager sg(ctx);
  int32_t* dml;
  GH_TRY(sg.out(match_row, (size_t)L->ks, &dml));
  double Rt16[16];
  int32_t n_iter = 0, conv = 0;
  gh_loop_job J;
  memset(&J, 0, sizeof(J));
  J.p = &p; J.kpS = L->kpS.as<double>(); J.ks = L->ks; J.kpT = L->kpT.as<double>(); J.kt = L->kt; J.FD = L->FD.p; J.Rt16 = Rt16;
  J.n_iter = &n_iter; J.converged = &conv; J.matchlist = dml; J.ml_row0 = p.max_iter - 1;
  J.resume_in = L->started ? &L->st : nullptr; J.resume_out = &L->st; J.kpS_out = L->kpS.as<double>(); J.trace_last = out;
  memset(out, 0, sizeof(*out));
  GH_TRY(gh_register_batch_dev(ctx, 1, &J));
  GH_HIP(hipStreamSynchronize(ctx->stream));
  L->started = true;
  if (L->ks <= 0 || L->kt <= 0 || conv) L->finished = true;
  if (L->ks <= 0 || L->kt <= 0) out->converged = 1;
  return sg.finish();
}

extern "C" int ghicp_loop_result(const ghicp_loop* L, double* Rt16, int32_t* n_iter, int32_t* converged, double* rmse_after) {
  if (!L || !Rt16) return GHICP_ERR_ARG;
  for (int d = 0; d < 16; d++) Rt16[d] = L->started ? L->st.Rt_till[d] : (d % 5 == 0 ? 1.0 : 0.0);
  if (n_iter) *n_iter = L->started ? L->st.it : 0;
  if (converged) *converged = L->started ? L->st.converged_flag : 0;
  if (rmse_after) *rmse_after = L->started ? L->st.rmse_after : 0.0;
  return GHICP_OK;
}

extern "C" void ghicp_loop_destroy(ghicp_loop* L) {
  if (!L) return;
  (void)hipSetDevice(L->ctx->device);
  L->kpS.release(); L->kpT.release(); L->FD.release();
  delete L;
}
