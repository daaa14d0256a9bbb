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
// frozen (icp_frozen): its blocks return before they touch anything.  Per iteration the host reads one byte per pair.  No float atomics: the
// integer counters are those of the single-pair kernels.
//   ghicp_refine_clouds_reciprocal  the same driver (refine_clouds_impl) with use_reciprocal honoured: after every forward search the reciprocal
//                               test of all running pairs of the chunk, in one launch sequence and without a host wait (refine_recip.hip)
#include "cloud.h"
#include "refine_dev.h"
#include "refine_plan.h"

namespace {

using namespace icpdev;
using namespace rfdev;

__device__ inline double* part_of(const RefineArgs& A, unsigned p) { return A.part + (size_t)p * NBLK * NPART; }
__device__ inline unsigned* hist_of(const RefineArgs& A, unsigned p) { return A.hist + (size_t)p * 6 * SEL_BINS; }

// cur = float(Rt_init) * source (ghicp_transform_cloud_f32); with_fin: final_transformation_ * that (the output cloud of ghicp_icp)
__global__ __launch_bounds__(256) void k_rf_transform(RefineArgs A, int with_fin) {
  const unsigned p = blockIdx.y;
  const RefinePair& D = A.pair[p];
  if (blockIdx.x * 256u >= (unsigned)D.ns) return;
  const IcpState* st = &A.st[p];
  if (st->refused) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= D.ns) return;
  const float4 S = D.src[i];
  float4 P = xf_point(D.init, S.x, S.y, S.z);
  if (with_fin) P = xf_point(st->fin, P.x, P.y, P.z);
  A.cur[D.off + i] = P;
}

__global__ __launch_bounds__(256) void k_rf_nn_fine(RefineArgs A, int final) {
  const unsigned p = blockIdx.y;
  const RefinePair& D = A.pair[p];
  if (blockIdx.x * 256u >= (unsigned)D.ns) return;
  const IcpState* st = &A.st[p];
  if (final ? st->refused != 0 : icp_frozen(st)) return;
  nn_fine_body(D.X.fine, A.cur + D.off, D.ns, blockIdx.x * 256 + threadIdx.x, A.nn + D.off, A.nd + D.off, A.pend + D.off, &A.pendc[p]);
}

__global__ __launch_bounds__(256) void k_rf_nn_coarse(RefineArgs A, int final) {
  const unsigned p = blockIdx.y;
  const RefinePair& D = A.pair[p];
  const unsigned nb = (unsigned)min(cdiv_dev(D.ns, 4), COARSE_BLK);
  if (blockIdx.x >= nb) return;
  const IcpState* st = &A.st[p];
  if (final ? st->refused != 0 : icp_frozen(st)) return;
  nn_coarse_body(D.X.coarse, A.cur + D.off, A.pend + D.off, A.pendc[p], blockIdx.x * 4u + (threadIdx.x >> 6), nb * 4u, A.nn + D.off, A.nd + D.off);
}

// calOverlap from the first search: a source point counts when its nearest target point lies at d^2 < thre_dis^2
__global__ __launch_bounds__(256) void k_rf_overlap(RefineArgs A, float r2) {
  const unsigned p = blockIdx.y;
  const RefinePair& D = A.pair[p];
  if (blockIdx.x * 256u >= (unsigned)D.ns) return;
  if (A.st[p].refused) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  block_count_add(i < D.ns && A.nd[D.off + i] < r2, &A.ovl[p]);
}

__global__ __launch_bounds__(256) void k_rf_corr_count(RefineArgs A) {
  const unsigned p = blockIdx.y;
  const RefinePair& D = A.pair[p];
  if (blockIdx.x * 256u >= (unsigned)D.ns) return;
  IcpState* st = &A.st[p];
  if (icp_frozen(st)) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  block_count_add(i < D.ns && A.nn[D.off + i] >= 0, &st->count);
}

__global__ __launch_bounds__(64) void k_rf_prep(RefineArgs A, int np) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= np || icp_frozen(&A.st[p])) return;
  icp_prep_body(&A.st[p]);
}

__global__ __launch_bounds__(256) void k_rf_sel_pass(RefineArgs A, int pass) {
  const unsigned p = blockIdx.y;
  const RefinePair& D = A.pair[p];
  const unsigned nblk = (unsigned)min(cdiv_dev(D.ns, 2048), 512);
  if (blockIdx.x >= nblk) return;
  IcpState* st = &A.st[p];
  if (icp_frozen(st)) return;
  sel_pass_body(pass, A.nn + D.off, A.nd + D.off, D.ns, st, hist_of(A, p), blockIdx.x, nblk);
}

__global__ __launch_bounds__(256) void k_rf_sel_final(RefineArgs A) {
  const unsigned p = blockIdx.x;
  IcpState* st = &A.st[p];
  if (icp_frozen(st)) return;
  sel_final_body(st, hist_of(A, p));
}

// W = 0: k_acc_means, 1: k_acc_cov, 2: k_acc_plane -- NBLK blocks per pair, as in the single-pair launch
template <int W>
__global__ __launch_bounds__(256) void k_rf_acc(RefineArgs A) {
  const unsigned p = blockIdx.y;
  const IcpState* st = &A.st[p];
  if (icp_frozen(st)) return;
  const RefinePair& D = A.pair[p];
  const CorrView V = {A.nn + D.off, A.nd + D.off, A.cur + D.off, D.tgt, D.ns};
  if (W == 0) acc_means_body(V, st, part_of(A, p), blockIdx.x);
  else if (W == 1) acc_cov_body(V, st, part_of(A, p), blockIdx.x);
  else acc_plane_body(V, D.tnrm, st, part_of(A, p), blockIdx.x);
}

__global__ __launch_bounds__(64) void k_rf_means(RefineArgs A) {
  const unsigned p = blockIdx.x;
  IcpState* st = &A.st[p];
  if (icp_frozen(st)) return;
  icp_means_body(st, part_of(A, p));
}

// the solve of every running pair, then the pair's byte of the status record
__global__ __launch_bounds__(64) void k_rf_step(RefineArgs A) {
  const unsigned p = blockIdx.x;
  IcpState* st = &A.st[p];
  if (!icp_frozen(st)) icp_step_body(st, part_of(A, p));
  if (threadIdx.x == 0) A.flag[p] = icp_frozen(st) ? 1 : 0;
}

// (a pair that converged in this iteration is not moved again: its points are rebuilt from the source for the output)
__global__ __launch_bounds__(256) void k_rf_apply(RefineArgs A) {
  const unsigned p = blockIdx.y;
  const RefinePair& D = A.pair[p];
  if (blockIdx.x * 256u >= (unsigned)D.ns) return;
  const IcpState* st = &A.st[p];
  if (icp_frozen(st)) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= D.ns) return;
  const float4 P = A.cur[D.off + i];
  A.cur[D.off + i] = xf_point(st->T, P.x, P.y, P.z);
}

__global__ __launch_bounds__(256) void k_rf_sum(RefineArgs A) {
  const unsigned p = blockIdx.y;
  if (A.st[p].refused) return;
  const RefinePair& D = A.pair[p];
  sum_f32_body(A.nd + D.off, D.ns, part_of(A, p), blockIdx.x);
}

// the NBLK block sums added one after the other, as ghicp_icp adds them on the host
__global__ __launch_bounds__(64) void k_rf_fitness(RefineArgs A, int np) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= np || A.st[p].refused) return;
  const double* part = part_of(A, (unsigned)p);
  double f = 0;
  for (int b = 0; b < NBLK; b++) f += part[b];
  A.st[p].fit_sum = f;
}

NnGrid nn_grid(const GridDesc& d, const DevBuf& pts, const DevBuf& start) { return NnGrid{d, pts.as<float4>(), start.as<unsigned>(), 1.0f / d.inv}; }

int nn_search_batch(ghicp_ctx* ctx, const RefineArgs& A, int np, int max_gs, int final) {
  hipStream_t s = ctx->stream;
  GH_HIP(hipMemsetAsync(A.pendc, 0, (size_t)np * sizeof(unsigned), s));
  hipLaunchKernelGGL(k_rf_nn_fine, dim3(max_gs, np), dim3(256), 0, s, A, final);
  hipLaunchKernelGGL(k_rf_nn_coarse, dim3(min(cdiv(max_gs * 256ll, 4), COARSE_BLK), np), dim3(256), 0, s, A, final);
  GH_HIP(hipGetLastError());
  return GHICP_OK;
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

// The body of both entry points (`who` names the one that was called).  recip_ok: use_reciprocal is honoured instead of refused.
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
  hipStream_t s = ctx->stream;
  const float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  size_t budget = (size_t)1 << 30;
#ifndef HIPSIM
  {
    size_t free_b = 0, total_b = 0;
    GH_HIP(hipMemGetInfo(&free_b, &total_b));
    budget = free_b / 2;
  }
#endif
  const std::vector<int> bounds = gh_refine_plan(n_pairs, ns_all.data(), max_concurrent, budget, recip ? kRecipPairBytes : kRefinePairBytes,
                                                 recip ? kRecipPointBytes : kRefinePointBytes);
  std::vector<RefinePair> hd;
  std::vector<IcpState> hs;
  std::vector<unsigned> hovl;
  for (size_t ch = 0; ch + 1 < bounds.size(); ch++) {
    const int b0 = bounds[ch], np = bounds[ch + 1] - b0;
    hd.assign((size_t)np, RefinePair());
    hs.assign((size_t)np, IcpState());
    long long npts = 0;
    int max_gs = 0, max_sel = 0, running = 0;
    for (int q = 0; q < np; q++) {
      const ghicp_cloud *a = S[b0 + q], *b = T[b0 + q];
      ghicp_refine_result& R = out[b0 + q];
      memset(&R, 0, sizeof(R));
      RefinePair& D = hd[q];
      memset(&D, 0, sizeof(D));
      for (int e = 0; e < 16; e++) D.init[e] = Rt_init ? (float)Rt_init[(size_t)(b0 + q) * 16 + e] : I16[e];
      mat4_to_result(I16, D.init, &R);
      IcpState& st = hs[q];
      memset(&st, 0, sizeof(st));
      memcpy(st.fin, I16, sizeof(I16));
      memcpy(st.T, I16, sizeof(I16));
      st.prev_mse = 1.7976931348623157e308;
      st.eps_t = P->transformation_epsilon;
      st.eps_e = P->euclidean_fitness_epsilon;
      st.max_iter = P->max_iter;
      st.metric = P->metric;
      st.ratio = 1.0f;
      D.ns = (int)a->m;
      D.off = npts;
      if (a->m == 0 || b->m == 0) {  // nothing to launch: ghicp_icp's answers for an empty cloud
        st.refused = 1;
        D.ns = 0;
        float ratio = 1.0f;
        if (P->use_trimmed) {
          ratio = a->m > 0 ? (float)((0.01 + 0) / (double)a->m) : 0.f;
          R.stats.overlap = ratio;
        }
        if (!(P->use_trimmed && ratio < P->min_overlap)) { R.stats.done = 1; R.stats.reason = GHICP_ICP_NO_CORRESPONDENCES; }
        continue;
      }
      D.X.fine = nn_grid(b->rf_fine, b->rf_fpts, b->rf_fstart);
      D.X.coarse = nn_grid(b->rf_coarse, b->rf_cpts, b->rf_cstart);
      D.tgt = b->ds.as<float4>();
      D.tnrm = plane ? b->rf_nrm.as<float>() : nullptr;
      D.src = a->ds.as<float4>();
      npts += a->m;
      max_gs = max(max_gs, cdiv(a->m, 256));
      max_sel = max(max_sel, min(cdiv(a->m, 2048), 512));
      running++;
    }
    if (running == 0) continue;
    RefineArgs A;
    memset(&A, 0, sizeof(A));
    RefinePair* dd;
    unsigned* misc;
    GH_TRY(ctx->reserve(B_RF_DESC, (size_t)np, &dd));
    GH_TRY(ctx->reserve(B_ICP_STATE, (size_t)np, &A.st));
    GH_TRY(ctx->reserve(B_ICP_CUR, (size_t)npts + 1, &A.cur));
    GH_TRY(ctx->reserve(B_ICP_NN, (size_t)npts + 1, &A.nn));
    GH_TRY(ctx->reserve(B_ICP_ND, (size_t)npts + 1, &A.nd));
    GH_TRY(ctx->reserve(B_ICP_PEND, (size_t)npts + 4, &A.pend));
    GH_TRY(ctx->reserve(B_ICP_PART, (size_t)np * NBLK * NPART, &A.part));
    if (P->use_trimmed) GH_TRY(ctx->reserve(B_ICP_KEYS, (size_t)np * 6 * SEL_BINS, &A.hist));
    GH_TRY(ctx->reserve(B_RF_MISC, (size_t)np * 3, &misc));
    A.pair = dd;
    A.pendc = misc;
    A.ovl = misc + np;
    A.flag = reinterpret_cast<unsigned char*>(misc + 2 * (size_t)np);
    RecipStage RS;
    if (recip) GH_TRY(gh_refine_recip_begin(ctx, hd.data(), np, npts, &RS));  // every buffer and the pairs' ranges of the cell table: before the loop
    hipEvent_t kt = ctx->kt_begin(KT_REFINE);
    GH_TRY(ctx->upload_table(hd.data(), (size_t)np * sizeof(RefinePair), dd));
    GH_TRY(ctx->upload_table(hs.data(), (size_t)np * sizeof(IcpState), A.st));
    hipLaunchKernelGGL(k_rf_transform, dim3(max_gs, np), dim3(256), 0, s, A, 0);
    // the first search serves the overlap gate and the first iteration: both see the untouched initial source
    GH_TRY(nn_search_batch(ctx, A, np, max_gs, 0));
    if (P->use_trimmed) {  // common_reg.cpp:64-74
      GH_HIP(hipMemsetAsync(A.ovl, 0, (size_t)np * sizeof(unsigned), s));
      hipLaunchKernelGGL(k_rf_overlap, dim3(max_gs, np), dim3(256), 0, s, A, P->thre_dis * P->thre_dis);
      hovl.assign((size_t)np, 0u);
      GH_HIP(hipMemcpyAsync(hovl.data(), A.ovl, (size_t)np * sizeof(unsigned), hipMemcpyDeviceToHost, s));
      GH_HIP(hipStreamSynchronize(s));
      running = 0;
      for (int q = 0; q < np; q++) {
        IcpState& st = hs[q];
        if (st.refused) continue;
        const float ratio = (float)((0.01 + (int)hovl[q]) / (double)hd[q].ns);  // common_reg.cpp:313
        out[b0 + q].stats.overlap = ratio;
        if (ratio < P->min_overlap) { st.refused = 1; continue; }  // "This registration would not be done"
        st.trimmed = ratio < 1.0f;
        st.ratio = ratio;
        running++;
      }
      GH_TRY(ctx->upload_table(hs.data(), (size_t)np * sizeof(IcpState), A.st));
    }
    unsigned char* pin = reinterpret_cast<unsigned char*>(ctx->pinned);
    static_assert(kRefineMaxChunk <= 4096, "one status byte per pair must fit the pinned scratch");
    bool have_nn = true;
    while (running > 0) {
      if (!have_nn) GH_TRY(nn_search_batch(ctx, A, np, max_gs, 0));
      have_nn = false;
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
      GH_HIP(hipGetLastError());
      GH_HIP(hipMemcpyAsync(pin, A.flag, (size_t)np, hipMemcpyDeviceToHost, s));
      GH_HIP(hipStreamSynchronize(s));
      running = 0;
      for (int q = 0; q < np; q++) running += pin[q] ? 0 : 1;
    }
    // output = final_transformation_ * input, then getFitnessScore() on it
    hipLaunchKernelGGL(k_rf_transform, dim3(max_gs, np), dim3(256), 0, s, A, 1);
    GH_TRY(nn_search_batch(ctx, A, np, max_gs, 1));
    hipLaunchKernelGGL(k_rf_sum, dim3(NBLK, np), dim3(256), 0, s, A);
    hipLaunchKernelGGL(k_rf_fitness, dim3(cdiv(np, 64)), dim3(64), 0, s, A, np);
    GH_HIP(hipGetLastError());
    GH_HIP(hipMemcpyAsync(hs.data(), A.st, (size_t)np * sizeof(IcpState), hipMemcpyDeviceToHost, s));
    ctx->kt_end(KT_REFINE, kt);
    GH_HIP(hipStreamSynchronize(s));
    for (int q = 0; q < np; q++) {
      const IcpState& st = hs[q];
      if (st.refused) continue;  // refused (or empty): T_icp = I, Rt_refined = the rounded init, filled above
      ghicp_refine_result& R = out[b0 + q];
      R.stats.done = 1;
      R.stats.iterations = st.iterations;
      R.stats.converged = st.converged;
      R.stats.reason = st.reason;
      R.stats.correspondences = st.nv;
      R.stats.mse = st.mse;
      R.stats.fitness = st.fit_sum / (double)hd[q].ns;
      mat4_to_result(st.fin, hd[q].init, &R);
    }
  }
  return GHICP_OK;
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
