// Batched fine registration over cached clouds: the loop of ghicp_icp (icp.hip) for MANY pairs of ghicp_cloud handles in one launch
// sequence per iteration -- the fine stage after ghicp_register_clouds (coarse-to-fine; the reference documents ICP of the down-sampled
// clouds from the GH-ICP pose as the next step, and runs it pair by pair).
//   ghicp_cloud_prepare_refine  once per cloud: the fine + coarse 1-NN grids over its down-sampled points and, for point-to-plane, its
//                               k-NN normals, kept in buffers of the handle (ghicp_icp rebuilds both for every pair)
//   ghicp_refine_clouds         per chunk of pairs: the pairs' working copies of their sources side by side in one cur / nn / nd array, one
//                               IcpState, NBLK partial records and 6 x SEL_BINS histogram words per pair.  Every kernel of the single-pair loop has
//                               a batched form k_rf_* on a 2-D grid: blockIdx.y is the pair, blockIdx.x the block WITHIN the pair, so no block spans
//                               two pairs and a pair sees the block count, the strides and the reduction order of its single-pair launch.  The bodies
//                               are the single-pair kernels' own (icp_dev.h): results are those of ghicp_icp bit for bit.
// blockIdx.y is uniform over the block, so the descriptor reads below are scalar loads, once per block.  A pair that has left its loop is
// frozen (icpdev::frozen): its blocks return before they touch anything.  Per iteration the host reads one byte per pair.  No float atomics:
// the integer counters are those of the single-pair kernels.
//   ghicp_refine_clouds_reciprocal  the same method with use_reciprocal honoured: after every forward search the reciprocal test of all
//                               running pairs of the chunk, in one launch sequence and without a host wait (refine_recip.hip)
// What this loop shares with the batched generalized ICP lives in one place: the descriptors, the prologue of the 2-D launches and the
// kernels k_chunk_* (search, overlap count, fitness sum) in refine_dev.h, the chunk in flight (RfChunk) in refine_run.h.  Below: this method's
// kernels, its iteration, its results (IcpMethod), its argument checks.
#include "refine_run.h"

namespace {

using namespace icpdev;
using namespace rfdev;

__device__ inline unsigned* hist_of(const RefineArgs& A, unsigned p) { return A.hist + (size_t)p * 6 * SEL_BINS; }

// cur = float(Rt_init) * source (ghicp_transform_cloud_f32); with_fin: final_transformation_ * that (the output cloud of ghicp_icp)
__global__ __launch_bounds__(256) void k_rf_transform(RefineArgs A, int with_fin) {
  const RefinePair& D = A.pair[blockIdx.y];
  if (!point_block(D.ns, &A.st[blockIdx.y], 1)) return;
  const IcpState* st = &A.st[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= D.ns) return;
  const float4 S = D.src[i];
  float4 P = xf_point(D.init, S.x, S.y, S.z);
  if (with_fin) P = xf_point(st->fin, P.x, P.y, P.z);
  A.cur[D.off + i] = P;
}

__global__ __launch_bounds__(256) void k_rf_corr_count(RefineArgs A) {
  const RefinePair& D = A.pair[blockIdx.y];
  if (!point_block(D.ns, &A.st[blockIdx.y])) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  block_count_add(i < D.ns && A.nn[D.off + i] >= 0, &A.st[blockIdx.y].count);
}

__global__ __launch_bounds__(64) void k_rf_prep(RefineArgs A, int np) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= np || frozen(&A.st[p])) return;
  icp_prep_body(&A.st[p]);
}

__global__ __launch_bounds__(256) void k_rf_sel_pass(RefineArgs A, int pass) {
  const unsigned p = blockIdx.y;
  const RefinePair& D = A.pair[p];
  const unsigned nblk = (unsigned)min(cdiv_dev(D.ns, 2048), 512);
  if (blockIdx.x >= nblk) return;
  IcpState* st = &A.st[p];
  if (frozen(st)) return;
  sel_pass_body(pass, A.nn + D.off, A.nd + D.off, D.ns, st, hist_of(A, p), blockIdx.x, nblk);
}

__global__ __launch_bounds__(256) void k_rf_sel_final(RefineArgs A) {
  const unsigned p = blockIdx.x;
  IcpState* st = &A.st[p];
  if (frozen(st)) return;
  sel_final_body(st, hist_of(A, p));
}

// W = 0: k_acc_means, 1: k_acc_cov, 2: k_acc_plane -- NBLK blocks per pair, as in the single-pair launch
template <int W>
__global__ __launch_bounds__(256) void k_rf_acc(RefineArgs A) {
  const unsigned p = blockIdx.y;
  const IcpState* st = &A.st[p];
  if (frozen(st)) return;
  const RefinePair& D = A.pair[p];
  const CorrView V = {A.nn + D.off, A.nd + D.off, A.cur + D.off, D.tgt, D.ns};
  if (W == 0) acc_means_body(V, st, part_of(A, p), blockIdx.x);
  else if (W == 1) acc_cov_body(V, st, part_of(A, p), blockIdx.x);
  else acc_plane_body(V, D.tnrm, st, part_of(A, p), blockIdx.x);
}

__global__ __launch_bounds__(64) void k_rf_means(RefineArgs A) {
  const unsigned p = blockIdx.x;
  IcpState* st = &A.st[p];
  if (frozen(st)) return;
  icp_means_body(st, part_of(A, p));
}

// the solve of every running pair, then the pair's byte of the status record
__global__ __launch_bounds__(64) void k_rf_step(RefineArgs A) {
  const unsigned p = blockIdx.x;
  IcpState* st = &A.st[p];
  if (!frozen(st)) icp_step_body(st, part_of(A, p));
  if (threadIdx.x == 0) A.flag[p] = frozen(st) ? 1 : 0;
}

// (a pair that converged in this iteration is not moved again: its points are rebuilt from the source for the output)
__global__ __launch_bounds__(256) void k_rf_apply(RefineArgs A) {
  const RefinePair& D = A.pair[blockIdx.y];
  if (!point_block(D.ns, &A.st[blockIdx.y])) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= D.ns) return;
  const float4 P = A.cur[D.off + i];
  A.cur[D.off + i] = xf_point(A.st[blockIdx.y].T, P.x, P.y, P.z);
}

void mat4_to_result(const float* T_icp, const float* init_f, ghicp_refine_result* r) {
  memcpy(r->T_icp, T_icp, 16 * sizeof(float));
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      double s = 0;
      for (int k = 0; k < 4; k++) s += (double)T_icp[i * 4 + k] * (double)init_f[k * 4 + j];
      r->Rt_refined[i * 4 + j] = s;
    }
}

const float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

// What RfChunk (refine_run.h) asks of a method: the loop of ghicp_icp
struct IcpMethod {
  typedef RefineArgs Args;
  typedef ghicp_refine_result Result;
  typedef ghicp_icp_params Params;
  static constexpr int TIMER = KT_REFINE;
  typedef RfChunk<IcpMethod> Chunk;
  const ghicp_icp_params* P;
  bool plane, recip;
  RecipStage RS;

  void pair(const ghicp_cloud*, const ghicp_cloud* b, RefinePair& D, IcpState& st, ghicp_refine_result& R) const {
    mat4_to_result(I16, D.init, &R);  // a refused pair: T_icp = I, Rt_refined = the rounded init
    memcpy(st.fin, I16, sizeof(I16));
    memcpy(st.T, I16, sizeof(I16));
    st.prev_mse = 1.7976931348623157e308;
    st.eps_t = P->transformation_epsilon;
    st.eps_e = P->euclidean_fitness_epsilon;
    st.max_iter = P->max_iter;
    st.metric = P->metric;
    st.ratio = 1.0f;
    D.tnrm = plane ? b->rf_nrm.as<float>() : nullptr;
  }

  int reserve(Chunk& C, ReserveAt at) {
    if (at == RESERVE_PER_PAIR && P->use_trimmed) return C.ctx->reserve(B_ICP_KEYS, (size_t)C.np * 6 * SEL_BINS, &C.A.hist);
    if (at == RESERVE_LAST && recip) return gh_refine_recip_begin(C.ctx, C.hd.data(), C.np, C.npts, &RS);  // every buffer and the pairs' ranges of the cell table: before the loop
    return GHICP_OK;
  }

  void accept(IcpState& st, float ratio) const {
    st.trimmed = ratio < 1.0f;
    st.ratio = ratio;
  }

  // the loop moves cur at the end of an iteration (k_rf_apply); the first search and the output cloud are built from the source
  int search(Chunk& C, SearchPhase ph) const {
    if (ph != SEARCH_LOOP) hipLaunchKernelGGL(k_rf_transform, dim3(C.max_gs, C.np), dim3(256), 0, C.s, C.A, ph == SEARCH_FINAL ? 1 : 0);
    return C.nn_search(ph == SEARCH_FINAL ? 1 : 0);
  }

  int iteration(Chunk& C) const {
    const RefineArgs& A = C.A;
    const int np = C.np, max_gs = C.max_gs;
    const int max_sel = min(cdiv(max_gs, 8), 512);  // blocks of the radix select of the largest source: min(cdiv(ns, 2048), 512)
    ghicp_ctx* ctx = C.ctx;
    hipStream_t s = C.s;
    if (recip) GH_TRY(gh_refine_recip_step(ctx, A, RS, np, max_gs));  // determineReciprocalCorrespondences: after the search (and the overlap gate)
    hipLaunchKernelGGL(k_rf_corr_count, dim3(max_gs, np), dim3(256), 0, s, A);
    hipLaunchKernelGGL(k_rf_prep, dim3(cdiv(np, 64)), dim3(64), 0, s, A, np);
    if (P->use_trimmed) {
      GH_HIP(hipMemsetAsync(A.hist, 0, (size_t)np * 6 * SEL_BINS * sizeof(unsigned), s));
      for (int pass = 0; pass < 6; pass++) hipLaunchKernelGGL(k_rf_sel_pass, dim3(max_sel, np), dim3(256), 0, s, A, pass);
      hipLaunchKernelGGL(k_rf_sel_final, dim3(np), dim3(256), 0, s, A);
    }
    if (!plane) {
      hipLaunchKernelGGL(k_rf_acc<0>, dim3(NBLK, np), dim3(256), 0, s, A);
      hipLaunchKernelGGL(k_rf_means, dim3(np), dim3(64), 0, s, A);
      hipLaunchKernelGGL(k_rf_acc<1>, dim3(NBLK, np), dim3(256), 0, s, A);
    } else {
      hipLaunchKernelGGL(k_rf_acc<2>, dim3(NBLK, np), dim3(256), 0, s, A);
    }
    hipLaunchKernelGGL(k_rf_step, dim3(np), dim3(64), 0, s, A);
    hipLaunchKernelGGL(k_rf_apply, dim3(max_gs, np), dim3(256), 0, s, A);
    return GHICP_OK;
  }

  void result(const IcpState& st, const RefinePair& D, ghicp_refine_result& R) const {
    R.stats.correspondences = st.nv;
    mat4_to_result(st.fin, D.init, &R);
  }
};

}  // namespace

int gh_cloud_build_grids(ghicp_ctx* ctx, ghicp_cloud* c) {
  hipStream_t s = ctx->stream;
  memset(&c->rf_fine, 0, sizeof(GridDesc));
  memset(&c->rf_coarse, 0, sizeof(GridDesc));
  if (c->m <= 0) return GHICP_OK;
  icpdev::NnIndex X;
  GH_TRY(gh_icp_build_index(ctx, reinterpret_cast<const float*>(c->ds.p), c->m, 4, &X));
  // out of the context's grid buffers into the handle's own
  GH_HIP(c->rf_fpts.reserve((size_t)c->m * sizeof(float4)));
  GH_HIP(c->rf_cpts.reserve((size_t)c->m * sizeof(float4)));
  GH_HIP(c->rf_fstart.reserve(((size_t)X.fine.d.ncell + 1) * sizeof(unsigned)));
  GH_HIP(c->rf_cstart.reserve(((size_t)X.coarse.d.ncell + 1) * sizeof(unsigned)));
  GH_HIP(hipMemcpyAsync(c->rf_fpts.p, X.fine.pts, (size_t)c->m * sizeof(float4), hipMemcpyDeviceToDevice, s));
  GH_HIP(hipMemcpyAsync(c->rf_cpts.p, X.coarse.pts, (size_t)c->m * sizeof(float4), hipMemcpyDeviceToDevice, s));
  GH_HIP(hipMemcpyAsync(c->rf_fstart.p, X.fine.start, ((size_t)X.fine.d.ncell + 1) * sizeof(unsigned), hipMemcpyDeviceToDevice, s));
  GH_HIP(hipMemcpyAsync(c->rf_cstart.p, X.coarse.start, ((size_t)X.coarse.d.ncell + 1) * sizeof(unsigned), hipMemcpyDeviceToDevice, s));
  c->rf_fine = X.fine.d;
  c->rf_coarse = X.coarse.d;
  return GHICP_OK;
}

extern "C" int ghicp_cloud_prepare_refine(ghicp_cloud* c, int32_t covariance_k) {
  if (!c || !c->ctx) return GHICP_ERR_ARG;
  ghicp_ctx* ctx = c->ctx;
  GH_ENTER(ctx);
  GH_ARG(covariance_k >= 0 && covariance_k <= 20);
  if (!c->ds.p) return ctx->fail(GHICP_ERR_ARG, "ghicp_cloud_prepare_refine: this handle was rebuilt from stored features and holds no points");
  hipStream_t s = ctx->stream;
  const float* ds = reinterpret_cast<const float*>(c->ds.p);
  const bool had_grids = c->rf_ready;
  const int had_k = c->rf_k;
  c->rf_invalidate();  // until everything below is in place
  if (!had_grids) GH_TRY(gh_cloud_build_grids(ctx, c));
  if (covariance_k > 0 && (covariance_k != had_k || !had_grids)) {
    GH_HIP(c->rf_nrm.reserve(((size_t)c->m * 3 + 3) * sizeof(float)));
    GH_TRY(gh_knn_normals_dev(ctx, ds, c->m, 4, covariance_k, c->rf_nrm.as<float>()));
  }
  GH_HIP(hipStreamSynchronize(s));  // afterwards the handle may serve any context of the device
  c->rf_k = covariance_k;
  c->rf_ready = true;
  return GHICP_OK;
}

namespace {

#define RF_ARG(cond)                                                                   \
  do {                                                                                 \
    if (!(cond)) return ctx->fail(GHICP_ERR_ARG, "%s: bad argument (%s)", who, #cond); \
  } while (0)

// The body of both entry points (`who` names the one that was called): the argument checks, then the chunks.  recip_ok: use_reciprocal is
// honoured instead of refused.
int refine_clouds_impl(ghicp_ctx* ctx, const char* who, bool recip_ok, const ghicp_icp_params* P, int32_t n_pairs, const ghicp_cloud* const* S,
                       const ghicp_cloud* const* T, const double* Rt_init, int32_t max_concurrent, ghicp_refine_result* out) {
  RF_ARG(P != nullptr && n_pairs >= 0 && max_concurrent >= 0 && (n_pairs == 0 || (S != nullptr && T != nullptr && out != nullptr)));
  RF_ARG(P->metric == GHICP_ICP_POINT_TO_POINT || P->metric == GHICP_ICP_POINT_TO_PLANE);
  if (P->use_reciprocal && !recip_ok)
    return ctx->fail(GHICP_ERR_ARG, "%s: reciprocal correspondences are not covered by this call (use ghicp_refine_clouds_reciprocal or ghicp_icp)", who);
  const bool recip = P->use_reciprocal != 0;
  if (P->use_trimmed) RF_ARG(P->thre_dis > 0.f);
  const bool plane = P->metric == GHICP_ICP_POINT_TO_PLANE;
  if (plane) RF_ARG(P->covariance_k >= 1 && P->covariance_k <= 20);
  // every pair is checked before anything is written or launched
  std::vector<int64_t> ns_all((size_t)n_pairs);
  for (int i = 0; i < n_pairs; i++) {
    const ghicp_cloud *a = S[i], *b = T[i];
    RF_ARG(a != nullptr && b != nullptr && a->ctx && b->ctx && a->ctx->device == ctx->device && b->ctx->device == ctx->device);
    if (!a->ds.p) return ctx->fail(GHICP_ERR_ARG, "%s: the source of pair %d was rebuilt from stored features and holds no points", who, i);
    if (!b->rf_ready) return ctx->fail(GHICP_ERR_ARG, "%s: the target of pair %d is not prepared (ghicp_cloud_prepare_refine)", who, i);
    if (plane && b->rf_k != P->covariance_k)
      return ctx->fail(GHICP_ERR_ARG, "%s: the target of pair %d holds normals for k = %d, the parameters ask for k = %d", who, i, b->rf_k, P->covariance_k);
    ns_all[i] = a->m;
  }
  if (n_pairs == 0) return GHICP_OK;
  size_t budget;
  GH_TRY(refine_budget(ctx, &budget));
  IcpMethod M = {P, plane, recip, {}};
  return IcpMethod::Chunk(ctx, M, P, S, T, Rt_init, out)
      .run(gh_refine_plan(n_pairs, ns_all.data(), max_concurrent, budget, recip ? kRecipPairBytes : kRefinePairBytes, recip ? kRecipPointBytes : kRefinePointBytes));
}

}  // namespace

extern "C" int ghicp_refine_clouds(ghicp_ctx* ctx, const ghicp_icp_params* P, int32_t n_pairs, const ghicp_cloud* const* S, const ghicp_cloud* const* T,
                                   const double* Rt_init, int32_t max_concurrent, ghicp_refine_result* out) {
  GH_ENTER(ctx);
  return refine_clouds_impl(ctx, "ghicp_refine_clouds", false, P, n_pairs, S, T, Rt_init, max_concurrent, out);
}

extern "C" int ghicp_refine_clouds_reciprocal(ghicp_ctx* ctx, const ghicp_icp_params* P, int32_t n_pairs, const ghicp_cloud* const* S,
                                              const ghicp_cloud* const* T, const double* Rt_init, int32_t max_concurrent, ghicp_refine_result* out) {
  GH_ENTER(ctx);
  return refine_clouds_impl(ctx, "ghicp_refine_clouds_reciprocal", true, P, n_pairs, S, T, Rt_init, max_concurrent, out);
}
