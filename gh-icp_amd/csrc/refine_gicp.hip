// Batched generalized ICP over cached clouds: the loop of ghicp_gicp_from (icp.hip) for MANY pairs of ghicp_cloud handles in one launch
// sequence per outer iteration -- the batched ICP's shape (refine.hip) for CRegistration::gicp_reg.
//   ghicp_cloud_prepare_gicp  once per cloud: the regularised k-NN covariances of its down-sampled points, in the cloud's own frame, and the
//                             1-NN grids of ghicp_cloud_prepare_refine, kept in buffers of the handle (ghicp_gicp recomputes the
//                             covariances of both clouds and the grids of the target for every pair)
//   ghicp_gicp_clouds         per chunk of pairs: the pairs' moved sources side by side in one cur / nn / nd / mahal array, one GicpState and
//                             NBLK partial records per pair.  Every kernel of the single-pair loop has a batched form k_gb_* on a 2-D grid:
//                             blockIdx.y is the pair, blockIdx.x the block WITHIN the pair, so no block spans two pairs and a pair sees the
//                             block count (NBLK, cdiv(ns, 256)), the strides and the reduction order of its single-pair launch.  The bodies
//                             are the single-pair kernels' own (icp_dev.h): results are those of ghicp_gicp_from bit for bit.
// blockIdx.y is uniform over the block, so the descriptor reads below are scalar loads, once per block.  A pair that has left its loop is
// frozen (icpdev::frozen): its blocks return before they touch anything; within an outer iteration inner_done stops a pair's inner steps as
// in the single-pair loop.  Per outer iteration the host reads one byte per pair.  No float atomics.
// What this loop shares with the batched ICP lives in one place: the descriptors, the prologue of the 2-D launches and the kernels
// k_chunk_* (search, overlap count, fitness sum) in refine_dev.h, the chunk in flight (RfChunk) in refine_run.h.  Below: this method's
// kernels, its iteration, its results (GicpMethod), its argument checks.
#include "refine_run.h"

namespace {

using namespace icpdev;
using namespace rfdev;

// cur = transformation_ * source.  final: for every pair that ran (the output cloud), else for the pairs still in their loop
__global__ __launch_bounds__(256) void k_gb_apply(GicpArgs A, int final) {
  const GicpPair& D = A.pair[blockIdx.y];
  if (!point_block(D.ns, &A.st[blockIdx.y], final)) return;
  gicp_apply_body(D.src, D.ns, blockIdx.x * 256 + threadIdx.x, &A.st[blockIdx.y], A.cur + D.off);
}

// NBLK blocks per pair, as in the single-pair launch
__global__ __launch_bounds__(256) void k_gb_mahal(GicpArgs A) {
  const unsigned p = blockIdx.y;
  const GicpState* st = &A.st[p];
  if (frozen(st)) return;
  const GicpPair& D = A.pair[p];
  gicp_mahal_body(A.nn + D.off, A.nd + D.off, D.ns, D.covS, D.covT, st, A.mahal + D.off * 6, part_of(A, p), blockIdx.x);
}

__global__ __launch_bounds__(64) void k_gb_prep(GicpArgs A) {
  const unsigned p = blockIdx.x;
  GicpState* st = &A.st[p];
  if (frozen(st)) return;
  gicp_prep_body(st, part_of(A, p));
}

__global__ __launch_bounds__(256) void k_gb_acc(GicpArgs A) {
  const unsigned p = blockIdx.y;
  const GicpState* st = &A.st[p];
  if (frozen(st)) return;
  const GicpPair& D = A.pair[p];
  gicp_acc_body(D.src, D.tgt, A.nn + D.off, D.ns, A.mahal + D.off * 6, st, part_of(A, p), blockIdx.x);
}

__global__ __launch_bounds__(64) void k_gb_solve(GicpArgs A) {
  const unsigned p = blockIdx.x;
  GicpState* st = &A.st[p];
  if (frozen(st)) return;
  gicp_solve_body(st, part_of(A, p));
}

// the delta test of every running pair, then the pair's byte of the status record
__global__ __launch_bounds__(64) void k_gb_outer(GicpArgs A, int np) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= np) return;
  GicpState* st = &A.st[p];
  if (!frozen(st)) gicp_outer_body(st);
  A.flag[p] = frozen(st) ? 1 : 0;
}

// What RfChunk (refine_run.h) asks of a method: the loop of ghicp_gicp_from
struct GicpMethod {
  typedef GicpArgs Args;
  typedef ghicp_gicp_result Result;
  typedef ghicp_gicp_params Params;
  static constexpr int TIMER = KT_GICP_CLOUDS;
  typedef RfChunk<GicpMethod> Chunk;
  const ghicp_gicp_params* P;

  void pair(const ghicp_cloud* a, const ghicp_cloud* b, GicpPair& D, GicpState& st, ghicp_gicp_result& R) const {
    memcpy(R.T, D.init, sizeof(D.init));  // a refused pair: T = the rounded init
    memcpy(st.T, D.init, sizeof(D.init));
    st.maxd2 = P->max_correspondence_distance * P->max_correspondence_distance;
    st.inv_eps_r = 1.0 / P->rotation_epsilon;
    st.inv_eps_t = 1.0 / P->transformation_epsilon;
    st.max_iter = P->max_iter;
    D.covT = b->gc_cov.as<double>();
    D.covS = a->gc_cov.as<double>();
  }

  int reserve(Chunk& C, ReserveAt at) const { return at == RESERVE_PER_POINT ? C.ctx->reserve(B_GICP_MAHAL, (size_t)C.npts * 6 + 6, &C.A.mahal) : GHICP_OK; }

  void accept(GicpState&, float) const {}  // use_trimmed acts as the gate only

  // every search is of the source under the pair's current transformation_
  int search(Chunk& C, SearchPhase ph) const {
    const int final = ph == SEARCH_FINAL ? 1 : 0;
    return C.nn_search(final, [&] { hipLaunchKernelGGL(k_gb_apply, dim3(C.max_gs, C.np), dim3(256), 0, C.s, C.A, final); });
  }

  int iteration(Chunk& C) const {
    const GicpArgs& A = C.A;
    const int np = C.np;
    hipStream_t s = C.s;
    hipLaunchKernelGGL(k_gb_mahal, dim3(NBLK, np), dim3(256), 0, s, A);
    hipLaunchKernelGGL(k_gb_prep, dim3(np), dim3(64), 0, s, A);
    for (int k = 0; k < P->max_inner_iter; k++) {
      hipLaunchKernelGGL(k_gb_acc, dim3(NBLK, np), dim3(256), 0, s, A);
      hipLaunchKernelGGL(k_gb_solve, dim3(np), dim3(64), 0, s, A);
    }
    hipLaunchKernelGGL(k_gb_outer, dim3(cdiv(np, 64)), dim3(64), 0, s, A, np);
    return GHICP_OK;
  }

  void result(const GicpState& st, const GicpPair&, ghicp_gicp_result& R) const {
    R.stats.correspondences = st.count;
    memcpy(R.T, st.T, sizeof(st.T));
  }
};

bool holds_cov(const ghicp_cloud* c, const ghicp_gicp_params* P) { return c->gc_ready && c->gc_k == P->covariance_k && c->gc_eps == P->gicp_epsilon; }

}  // namespace

extern "C" int ghicp_cloud_prepare_gicp(ghicp_cloud* c, int32_t covariance_k, double gicp_epsilon) {
  if (!c || !c->ctx) return GHICP_ERR_ARG;
  ghicp_ctx* ctx = c->ctx;
  GH_ENTER(ctx);
  GH_ARG(covariance_k >= 1 && covariance_k <= 20 && gicp_epsilon > 0.0);
  if (!c->ds.p) return ctx->fail(GHICP_ERR_ARG, "ghicp_cloud_prepare_gicp: this handle was rebuilt from stored features and holds no points");
  const bool had_grids = c->rf_ready;
  const bool had_cov = c->gc_ready && c->gc_k == covariance_k && c->gc_eps == gicp_epsilon;
  c->gc_invalidate();  // until everything below is in place
  if (!had_grids) {
    c->rf_invalidate();
    GH_TRY(gh_cloud_build_grids(ctx, c));
  }
  if (!had_cov && c->m > 0) {
    GH_HIP(c->gc_cov.reserve(((size_t)c->m * 6 + 6) * sizeof(double)));
    GH_TRY(gh_gicp_cov_dev(ctx, reinterpret_cast<const float*>(c->ds.p), c->m, 4, covariance_k, gicp_epsilon, c->gc_cov.as<double>()));
  }
  GH_HIP(hipStreamSynchronize(ctx->stream));  // afterwards the handle may serve any context of the device
  if (!had_grids) c->rf_ready = true;  // (rf_k stays 0: no normals yet)
  c->gc_k = covariance_k;
  c->gc_eps = gicp_epsilon;
  c->gc_ready = true;
  return GHICP_OK;
}

extern "C" int ghicp_gicp_clouds(ghicp_ctx* ctx, const ghicp_gicp_params* P, int32_t n_pairs, const ghicp_cloud* const* S, const ghicp_cloud* const* T,
                                 const double* Rt_init, int32_t max_concurrent, ghicp_gicp_result* out) {
  GH_ENTER(ctx);
  GH_ARG(P != nullptr && n_pairs >= 0 && max_concurrent >= 0 && (n_pairs == 0 || (S != nullptr && T != nullptr && out != nullptr)));
  GH_ARG(P->covariance_k >= 1 && P->covariance_k <= 20 && P->max_inner_iter >= 1 && P->max_inner_iter <= 100);
  GH_ARG(P->max_correspondence_distance > 0.0 && P->gicp_epsilon > 0.0 && P->transformation_epsilon > 0.0 && P->rotation_epsilon > 0.0);
  if (P->use_trimmed) GH_ARG(P->thre_dis > 0.f);
  // every pair is checked before anything is written or launched
  std::vector<int64_t> ns_all((size_t)n_pairs);
  for (int i = 0; i < n_pairs; i++) {
    const ghicp_cloud *a = S[i], *b = T[i];
    GH_ARG(a != nullptr && b != nullptr && a->ctx && b->ctx && a->ctx->device == ctx->device && b->ctx->device == ctx->device);
    if (!a->ds.p || !b->ds.p) return ctx->fail(GHICP_ERR_ARG, "ghicp_gicp_clouds: a cloud of pair %d was rebuilt from stored features and holds no points", i);
    if (!holds_cov(a, P)) return ctx->fail(GHICP_ERR_ARG, "ghicp_gicp_clouds: the source of pair %d holds no covariances for k = %d, epsilon = %g (ghicp_cloud_prepare_gicp)", i, P->covariance_k, P->gicp_epsilon);
    if (!holds_cov(b, P)) return ctx->fail(GHICP_ERR_ARG, "ghicp_gicp_clouds: the target of pair %d holds no covariances for k = %d, epsilon = %g (ghicp_cloud_prepare_gicp)", i, P->covariance_k, P->gicp_epsilon);
    if (!b->rf_ready) return ctx->fail(GHICP_ERR_ARG, "ghicp_gicp_clouds: the target of pair %d holds no search grids (ghicp_cloud_prepare_gicp)", i);
    if (Rt_init) {
      const double* M = Rt_init + (size_t)i * 16;
      bool ok = true;
      for (int e = 0; e < 16; e++) ok = ok && std::isfinite((float)M[e]);
      if (!(ok && (float)M[12] == 0.f && (float)M[13] == 0.f && (float)M[14] == 0.f && (float)M[15] == 1.f))
        return ctx->fail(GHICP_ERR_ARG, "ghicp_gicp_clouds: Rt_init of pair %d has a non-finite entry or a last row other than (0, 0, 0, 1)", i);
    }
    ns_all[i] = a->m;
  }
  if (n_pairs == 0) return GHICP_OK;
  size_t budget;
  GH_TRY(refine_budget(ctx, &budget));
  GicpMethod M = {P};
  return GicpMethod::Chunk(ctx, M, P, S, T, Rt_init, out).run(gh_gicp_plan(n_pairs, ns_all.data(), max_concurrent, budget));
}
