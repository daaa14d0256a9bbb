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
//   ghicp_gicp_clouds_trimmed the loop of ghicp_gicp_trimmed_from in the same shape (GicpMethod<true>): between the search and k_gb_prep the
//                             distance rejection with its count (k_gb_reject), the rule and the radix select of the batched ICP over the survivors
//                             (k_gb_trim_prep, k_gb_sel_pass, k_gb_sel_final: the bodies of refine.hip's on the pair's GicpSel record, 6 x SEL_BINS
//                             histogram words per pair) and k_gb_mahal_trim in the place of k_gb_mahal.  A pair that keeps every survivor returns
//                             from the select passes at once.  The integer counters are those of the single-pair kernels; no further host wait.
#include <type_traits>

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

// ---- the trimmed loop's own kernels
__device__ inline unsigned* hist_of(const GicpTrimArgs& A, unsigned p) { return A.hist + (size_t)p * 6 * SEL_BINS; }

__global__ __launch_bounds__(256) void k_gb_reject(GicpTrimArgs A) {
  const GicpPair& D = A.pair[blockIdx.y];
  if (!point_block(D.ns, &A.st[blockIdx.y])) return;
  gicp_reject_body(A.nn + D.off, A.nd + D.off, D.ns, blockIdx.x * 256 + threadIdx.x, &A.st[blockIdx.y], &A.sel[blockIdx.y]);
}

__global__ __launch_bounds__(64) void k_gb_trim_prep(GicpTrimArgs A, int np) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= np || frozen(&A.st[p])) return;
  gicp_trim_prep_body(&A.st[p], &A.sel[p]);
}

// min(cdiv(ns, 2048), 512) blocks per pair, as in the single-pair launch
__global__ __launch_bounds__(256) void k_gb_sel_pass(GicpTrimArgs A, int pass) {
  const unsigned p = blockIdx.y;
  const GicpPair& D = A.pair[p];
  const unsigned nblk = (unsigned)min(cdiv_dev(D.ns, 2048), 512);
  if (blockIdx.x >= nblk) return;
  if (frozen(&A.st[p])) return;
  sel_pass_body(pass, A.nn + D.off, A.nd + D.off, D.ns, &A.sel[p], hist_of(A, p), blockIdx.x, nblk);
}

__global__ __launch_bounds__(256) void k_gb_sel_final(GicpTrimArgs A) {
  const unsigned p = blockIdx.x;
  if (frozen(&A.st[p])) return;
  sel_final_body(&A.sel[p], hist_of(A, p));
}

__global__ __launch_bounds__(256) void k_gb_mahal_trim(GicpTrimArgs A) {
  const unsigned p = blockIdx.y;
  const GicpState* st = &A.st[p];
  if (frozen(st)) return;
  const GicpPair& D = A.pair[p];
  gicp_mahal_trim_body(A.nn + D.off, A.nd + D.off, D.ns, D.covS, D.covT, st, &A.sel[p], A.mahal + D.off * 6, part_of(A, p), blockIdx.x);
}

// What RfChunk (refine_run.h) asks of a method: the loop of ghicp_gicp_from, or (TRIM) of ghicp_gicp_trimmed_from
template <bool TRIM>
struct GicpMethod {
  typedef typename std::conditional<TRIM, GicpTrimArgs, GicpArgs>::type Args;
  typedef ghicp_gicp_result Result;
  typedef ghicp_gicp_params Params;
  static constexpr int TIMER = KT_GICP_CLOUDS;
  typedef RfChunk<GicpMethod> Chunk;
  const ghicp_gicp_params* P;
  float trim_ratio;  // TRIM: in (0, 1] for every pair, or 0: each pair's own overlap estimate from the gate

  void pair(const ghicp_cloud* a, const ghicp_cloud* b, GicpPair& D, GicpState& st, ghicp_gicp_result& R) const {
    memcpy(R.T, D.init, sizeof(D.init));  // a refused pair: T = the rounded init
    memcpy(st.T, D.init, sizeof(D.init));
    st.maxd2 = P->max_correspondence_distance * P->max_correspondence_distance;
    st.inv_eps_r = 1.0 / P->rotation_epsilon;
    st.inv_eps_t = 1.0 / P->transformation_epsilon;
    st.max_iter = P->max_iter;
    st.ratio = TRIM ? trim_ratio : 0.f;
    D.covT = b->gc_cov.as<double>();
    D.covS = a->gc_cov.as<double>();
  }

  int reserve(Chunk& C, ReserveAt at) const {
    if (at == RESERVE_PER_POINT) return C.ctx->reserve(B_GICP_MAHAL, (size_t)C.npts * 6 + 6, &C.A.mahal);
    if constexpr (TRIM) {
      if (at == RESERVE_PER_PAIR) {  // the histograms where the batched ICP keeps its own
        GH_TRY(C.ctx->reserve(B_ICP_KEYS, (size_t)C.np * 6 * SEL_BINS, &C.A.hist));
        return C.ctx->reserve(B_GICP_SEL, (size_t)C.np, &C.A.sel);
      }
    }
    return GHICP_OK;
  }

  // untrimmed: use_trimmed acts as the gate only.  Trimmed with trim_ratio = 0: the pair's estimate feeds its rejector, as in icp_reg
  void accept(GicpState& st, float ratio) const {
    if (TRIM && trim_ratio == 0.f) st.ratio = ratio;
  }

  // every search is of the source under the pair's current transformation_
  int search(Chunk& C, SearchPhase ph) const {
    const int final = ph == SEARCH_FINAL ? 1 : 0;
    if constexpr (TRIM) {
      ghicp_ctx* ctx = C.ctx;
      if (ph == SEARCH_FIRST) GH_HIP(hipMemsetAsync(C.A.sel, 0, (size_t)C.np * sizeof(GicpSel), C.s));  // nothing counted yet
    }
    const GicpArgs& A = C.A;
    return C.nn_search(final, [&] { hipLaunchKernelGGL(k_gb_apply, dim3(C.max_gs, C.np), dim3(256), 0, C.s, A, final); });
  }

  int iteration(Chunk& C) const {
    const GicpArgs& A = C.A;
    const int np = C.np;
    hipStream_t s = C.s;
    // the correspondences of the iteration: their Mahalanobis matrices, their count and d^2 sum in the partial records
    if constexpr (TRIM) {
      const GicpTrimArgs& TA = C.A;
      const int max_sel = min(cdiv(C.max_gs, 8), 512);  // blocks of the radix select of the largest source: min(cdiv(ns, 2048), 512)
      ghicp_ctx* ctx = C.ctx;
      hipLaunchKernelGGL(k_gb_reject, dim3(C.max_gs, np), dim3(256), 0, s, TA);
      hipLaunchKernelGGL(k_gb_trim_prep, dim3(cdiv(np, 64)), dim3(64), 0, s, TA, np);
      hipEvent_t kt = ctx->kt_begin(KT_GICP_SELECT);
      GH_HIP(hipMemsetAsync(TA.hist, 0, (size_t)np * 6 * SEL_BINS * sizeof(unsigned), s));
      for (int pass = 0; pass < 6; pass++) hipLaunchKernelGGL(k_gb_sel_pass, dim3(max_sel, np), dim3(256), 0, s, TA, pass);
      hipLaunchKernelGGL(k_gb_sel_final, dim3(np), dim3(256), 0, s, TA);
      ctx->kt_end(KT_GICP_SELECT, kt);
      hipLaunchKernelGGL(k_gb_mahal_trim, dim3(NBLK, np), dim3(256), 0, s, TA);
    } else {
      hipLaunchKernelGGL(k_gb_mahal, dim3(NBLK, np), dim3(256), 0, s, A);
    }
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

namespace {

#define GB_ARG(cond)                                                                   \
  do {                                                                                 \
    if (!(cond)) return ctx->fail(GHICP_ERR_ARG, "%s: bad argument (%s)", who, #cond); \
  } while (0)

// The body of both entry points (`who` names the one that was called): the argument checks, then the chunks
template <bool TRIM>
int gicp_clouds_impl(ghicp_ctx* ctx, const char* who, const ghicp_gicp_params* P, int32_t n_pairs, const ghicp_cloud* const* S, const ghicp_cloud* const* T,
                     const double* Rt_init, float trim_ratio, int32_t max_concurrent, ghicp_gicp_result* out) {
  GB_ARG(P != nullptr && n_pairs >= 0 && max_concurrent >= 0 && (n_pairs == 0 || (S != nullptr && T != nullptr && out != nullptr)));
  GB_ARG(P->covariance_k >= 1 && P->covariance_k <= 20 && P->max_inner_iter >= 1 && P->max_inner_iter <= 100);
  GB_ARG(P->max_correspondence_distance > 0.0 && P->gicp_epsilon > 0.0 && P->transformation_epsilon > 0.0 && P->rotation_epsilon > 0.0);
  if (P->use_trimmed) GB_ARG(P->thre_dis > 0.f);
  if (TRIM) {
    GB_ARG(std::isfinite(trim_ratio) && trim_ratio >= 0.f && trim_ratio <= 1.f);
    if (trim_ratio == 0.f && !P->use_trimmed)
      return ctx->fail(GHICP_ERR_ARG, "%s: trim_ratio = 0 asks for the overlap estimate of the gate, which needs use_trimmed = 1", who);
  }
  // every pair is checked before anything is written or launched
  std::vector<int64_t> ns_all((size_t)n_pairs);
  for (int i = 0; i < n_pairs; i++) {
    const ghicp_cloud *a = S[i], *b = T[i];
    GB_ARG(a != nullptr && b != nullptr && a->ctx && b->ctx && a->ctx->device == ctx->device && b->ctx->device == ctx->device);
    if (!a->ds.p || !b->ds.p) return ctx->fail(GHICP_ERR_ARG, "%s: a cloud of pair %d was rebuilt from stored features and holds no points", who, i);
    if (!holds_cov(a, P)) return ctx->fail(GHICP_ERR_ARG, "%s: the source of pair %d holds no covariances for k = %d, epsilon = %g (ghicp_cloud_prepare_gicp)", who, i, P->covariance_k, P->gicp_epsilon);
    if (!holds_cov(b, P)) return ctx->fail(GHICP_ERR_ARG, "%s: the target of pair %d holds no covariances for k = %d, epsilon = %g (ghicp_cloud_prepare_gicp)", who, i, P->covariance_k, P->gicp_epsilon);
    if (!b->rf_ready) return ctx->fail(GHICP_ERR_ARG, "%s: the target of pair %d holds no search grids (ghicp_cloud_prepare_gicp)", who, i);
    if (Rt_init) {
      const double* M = Rt_init + (size_t)i * 16;
      bool ok = true;
      for (int e = 0; e < 16; e++) ok = ok && std::isfinite((float)M[e]);
      if (!(ok && (float)M[12] == 0.f && (float)M[13] == 0.f && (float)M[14] == 0.f && (float)M[15] == 1.f))
        return ctx->fail(GHICP_ERR_ARG, "%s: Rt_init of pair %d has a non-finite entry or a last row other than (0, 0, 0, 1)", who, i);
    }
    ns_all[i] = a->m;
  }
  if (n_pairs == 0) return GHICP_OK;
  size_t budget;
  GH_TRY(refine_budget(ctx, &budget));
  GicpMethod<TRIM> M = {P, trim_ratio};
  const std::vector<int> bounds = TRIM ? gh_gicp_trim_plan(n_pairs, ns_all.data(), max_concurrent, budget) : gh_gicp_plan(n_pairs, ns_all.data(), max_concurrent, budget);
  return typename GicpMethod<TRIM>::Chunk(ctx, M, P, S, T, Rt_init, out).run(bounds);
}

}  // namespace

extern "C" int ghicp_gicp_clouds(ghicp_ctx* ctx, const ghicp_gicp_params* P, int32_t n_pairs, const ghicp_cloud* const* S, const ghicp_cloud* const* T,
                                 const double* Rt_init, int32_t max_concurrent, ghicp_gicp_result* out) {
  GH_ENTER(ctx);
  return gicp_clouds_impl<false>(ctx, "ghicp_gicp_clouds", P, n_pairs, S, T, Rt_init, 0.f, max_concurrent, out);
}

extern "C" int ghicp_gicp_clouds_trimmed(ghicp_ctx* ctx, const ghicp_gicp_params* P, int32_t n_pairs, const ghicp_cloud* const* S, const ghicp_cloud* const* T,
                                         const double* Rt_init, float trim_ratio, int32_t max_concurrent, ghicp_gicp_result* out) {
  GH_ENTER(ctx);
  return gicp_clouds_impl<true>(ctx, "ghicp_gicp_clouds_trimmed", P, n_pairs, S, T, Rt_init, trim_ratio, max_concurrent, out);
}
