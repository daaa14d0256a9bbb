// Batched generalized ICP over cached clouds: the loop of ghicp_gicp_from (icp.hip) for MANY pairs of ghicp_cloud handles in one launch
// sequence per outer iteration -- refine.hip's shape for CRegistration::gicp_reg.
//   ghicp_cloud_prepare_gicp  once per cloud: the regularised k-NN covariances of its down-sampled points, in the cloud's own frame, and the
//                             1-NN grids of ghicp_cloud_prepare_refine, kept in buffers of the handle (ghicp_gicp recomputes the
//                             covariances of both clouds and the grids of the target for every pair)
//   ghicp_gicp_clouds         per chunk of pairs: the pairs' moved sources side by side in one cur / nn / nd / mahal array, one GicpState and
//                             NBLK partial records per pair.  Every kernel of the single-pair loop has a batched form k_gb_* on a 2-D grid:
//                             blockIdx.y is the pair, blockIdx.x the block WITHIN the pair, so no block spans two pairs and a pair sees the
//                             block count (NBLK, cdiv(ns, 256)), the strides and the reduction order of its single-pair launch.  The bodies
//                             are the single-pair kernels' own (icp_dev.h): results are those of ghicp_gicp_from bit for bit.
// blockIdx.y is uniform over the block, so the descriptor reads below are scalar loads, once per block.  A pair that has left its loop is
// frozen (gicp_frozen): its blocks return before they touch anything; within an outer iteration inner_done stops a pair's inner steps as
// in the single-pair loop.  Per outer iteration the host reads one byte per pair.  No float atomics.
#include "cloud.h"
#include "icp_dev.h"
#include "refine_plan.h"

namespace {

using namespace icpdev;

struct GicpPair {
  NnIndex X;           // the target's grids (buffers of its handle)
  const float4* tgt;   // the target's down-sampled points
  const double* covT;  // its covariances
  const float4* src;   // the source's down-sampled points
  const double* covS;  // its covariances, in the source's own frame
  long long off;       // the pair's slice of the concatenated per-point arrays
  int ns, pad_;
  float init[16];      // float(Rt_init): transformation_ before the first iteration
};

struct GicpArgs {
  const GicpPair* pair;
  GicpState* st;
  float4* cur;
  int* nn;
  float* nd;
  double* mahal;       // 6 per source point
  unsigned* pend;      // work lists of the coarse search, one slice per pair
  unsigned* pendc;     // their lengths
  unsigned* ovl;       // calOverlap counts
  double* part;        // NBLK x NPART per pair
  unsigned char* flag; // 1: the pair is frozen
};

constexpr int COARSE_BLK = 512;  // blocks per pair of the coarse search (any count gives the same result: one wave per query)

__device__ inline double* part_of(const GicpArgs& A, unsigned p) { return A.part + (size_t)p * NBLK * NPART; }

// cur = transformation_ * source.  final: for every pair that ran (the output cloud), else for the pairs still in their loop
__global__ __launch_bounds__(256) void k_gb_apply(GicpArgs A, int final) {
  const unsigned p = blockIdx.y;
  const GicpPair& D = A.pair[p];
  if (blockIdx.x * 256u >= (unsigned)D.ns) return;
  const GicpState* st = &A.st[p];
  if (final ? st->refused != 0 : gicp_frozen(st)) return;
  gicp_apply_body(D.src, D.ns, blockIdx.x * 256 + threadIdx.x, st, A.cur + D.off);
}

__global__ __launch_bounds__(256) void k_gb_nn_fine(GicpArgs A, int final) {
  const unsigned p = blockIdx.y;
  const GicpPair& D = A.pair[p];
  if (blockIdx.x * 256u >= (unsigned)D.ns) return;
  const GicpState* st = &A.st[p];
  if (final ? st->refused != 0 : gicp_frozen(st)) return;
  nn_fine_body(D.X.fine, A.cur + D.off, D.ns, blockIdx.x * 256 + threadIdx.x, A.nn + D.off, A.nd + D.off, A.pend + D.off, &A.pendc[p]);
}

__global__ __launch_bounds__(256) void k_gb_nn_coarse(GicpArgs A, int final) {
  const unsigned p = blockIdx.y;
  const GicpPair& D = A.pair[p];
  const unsigned nb = (unsigned)min(cdiv_dev(D.ns, 4), COARSE_BLK);
  if (blockIdx.x >= nb) return;
  const GicpState* st = &A.st[p];
  if (final ? st->refused != 0 : gicp_frozen(st)) return;
  nn_coarse_body(D.X.coarse, A.cur + D.off, A.pend + D.off, A.pendc[p], blockIdx.x * 4u + (threadIdx.x >> 6), nb * 4u, A.nn + D.off, A.nd + D.off);
}

// calOverlap from the first search: a (guess-moved) source point counts when its nearest target point lies at d^2 < thre_dis^2
__global__ __launch_bounds__(256) void k_gb_overlap(GicpArgs A, float r2) {
  const unsigned p = blockIdx.y;
  const GicpPair& D = A.pair[p];
  if (blockIdx.x * 256u >= (unsigned)D.ns) return;
  if (A.st[p].refused) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  block_count_add(i < D.ns && A.nd[D.off + i] < r2, &A.ovl[p]);
}

// NBLK blocks per pair, as in the single-pair launch
__global__ __launch_bounds__(256) void k_gb_mahal(GicpArgs A) {
  const unsigned p = blockIdx.y;
  const GicpState* st = &A.st[p];
  if (gicp_frozen(st)) return;
  const GicpPair& D = A.pair[p];
  gicp_mahal_body(A.nn + D.off, A.nd + D.off, D.ns, D.covS, D.covT, st, A.mahal + D.off * 6, part_of(A, p), blockIdx.x);
}

__global__ __launch_bounds__(64) void k_gb_prep(GicpArgs A) {
  const unsigned p = blockIdx.x;
  GicpState* st = &A.st[p];
  if (gicp_frozen(st)) return;
  gicp_prep_body(st, part_of(A, p));
}

__global__ __launch_bounds__(256) void k_gb_acc(GicpArgs A) {
  const unsigned p = blockIdx.y;
  const GicpState* st = &A.st[p];
  if (gicp_frozen(st)) return;
  const GicpPair& D = A.pair[p];
  gicp_acc_body(D.src, D.tgt, A.nn + D.off, D.ns, A.mahal + D.off * 6, st, part_of(A, p), blockIdx.x);
}

__global__ __launch_bounds__(64) void k_gb_solve(GicpArgs A) {
  const unsigned p = blockIdx.x;
  GicpState* st = &A.st[p];
  if (gicp_frozen(st)) return;
  gicp_solve_body(st, part_of(A, p));
}

// the delta test of every running pair, then the pair's byte of the status record
__global__ __launch_bounds__(64) void k_gb_outer(GicpArgs A, int np) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= np) return;
  GicpState* st = &A.st[p];
  if (!gicp_frozen(st)) gicp_outer_body(st);
  A.flag[p] = gicp_frozen(st) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_gb_sum(GicpArgs A) {
  const unsigned p = blockIdx.y;
  if (A.st[p].refused) return;
  const GicpPair& D = A.pair[p];
  sum_f32_body(A.nd + D.off, D.ns, part_of(A, p), blockIdx.x);
}

// the NBLK block sums added one after the other, as ghicp_gicp adds them on the host
__global__ __launch_bounds__(64) void k_gb_fitness(GicpArgs A, int np) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= np || A.st[p].refused) return;
  const double* part = part_of(A, (unsigned)p);
  double f = 0;
  for (int b = 0; b < NBLK; b++) f += part[b];
  A.st[p].fit_sum = f;
}

NnGrid nn_grid(const GridDesc& d, const DevBuf& pts, const DevBuf& start) { return NnGrid{d, pts.as<float4>(), start.as<unsigned>(), 1.0f / d.inv}; }

// transformation_ applied to the sources of the pairs, then their 1-NN in their targets
int move_and_search(ghicp_ctx* ctx, const GicpArgs& A, int np, int max_gs, int final) {
  hipStream_t s = ctx->stream;
  GH_HIP(hipMemsetAsync(A.pendc, 0, (size_t)np * sizeof(unsigned), s));
  hipLaunchKernelGGL(k_gb_apply, dim3(max_gs, np), dim3(256), 0, s, A, final);
  hipLaunchKernelGGL(k_gb_nn_fine, dim3(max_gs, np), dim3(256), 0, s, A, final);
  hipLaunchKernelGGL(k_gb_nn_coarse, dim3(min(cdiv(max_gs * 256ll, 4), COARSE_BLK), np), dim3(256), 0, s, A, final);
  GH_HIP(hipGetLastError());
  return GHICP_OK;
}

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
  const float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
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
  hipStream_t s = ctx->stream;
  size_t budget = (size_t)1 << 30;
#ifndef HIPSIM
  {
    size_t free_b = 0, total_b = 0;
    GH_HIP(hipMemGetInfo(&free_b, &total_b));
    budget = free_b / 2;
  }
#endif
  const std::vector<int> bounds = gh_gicp_plan(n_pairs, ns_all.data(), max_concurrent, budget);
  std::vector<GicpPair> hd;
  std::vector<GicpState> hs;
  std::vector<unsigned> hovl;
  for (size_t ch = 0; ch + 1 < bounds.size(); ch++) {
    const int b0 = bounds[ch], np = bounds[ch + 1] - b0;
    hd.assign((size_t)np, GicpPair());
    hs.assign((size_t)np, GicpState());
    long long npts = 0;
    int max_gs = 0, running = 0;
    for (int q = 0; q < np; q++) {
      const ghicp_cloud *a = S[b0 + q], *b = T[b0 + q];
      ghicp_gicp_result& R = out[b0 + q];
      memset(&R, 0, sizeof(R));
      GicpPair& D = hd[q];
      memset(&D, 0, sizeof(D));
      for (int e = 0; e < 16; e++) D.init[e] = Rt_init ? (float)Rt_init[(size_t)(b0 + q) * 16 + e] : I16[e];
      memcpy(R.T, D.init, sizeof(D.init));
      GicpState& st = hs[q];
      memset(&st, 0, sizeof(st));
      memcpy(st.T, D.init, sizeof(D.init));
      st.maxd2 = P->max_correspondence_distance * P->max_correspondence_distance;
      st.inv_eps_r = 1.0 / P->rotation_epsilon;
      st.inv_eps_t = 1.0 / P->transformation_epsilon;
      st.max_iter = P->max_iter;
      D.ns = (int)a->m;
      D.off = npts;
      if (a->m == 0 || b->m == 0) {  // nothing to launch: ghicp_gicp's answers for an empty cloud
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
      D.covT = b->gc_cov.as<double>();
      D.src = a->ds.as<float4>();
      D.covS = a->gc_cov.as<double>();
      npts += a->m;
      max_gs = max(max_gs, cdiv(a->m, 256));
      running++;
    }
    if (running == 0) continue;
    // everything the loop touches is reserved here: nothing allocates inside it
    GicpArgs A;
    memset(&A, 0, sizeof(A));
    GicpPair* dd;
    unsigned* misc;
    GH_TRY(ctx->reserve(B_RF_DESC, (size_t)np, &dd));
    GH_TRY(ctx->reserve(B_ICP_STATE, (size_t)np, &A.st));
    GH_TRY(ctx->reserve(B_ICP_CUR, (size_t)npts + 1, &A.cur));
    GH_TRY(ctx->reserve(B_ICP_NN, (size_t)npts + 1, &A.nn));
    GH_TRY(ctx->reserve(B_ICP_ND, (size_t)npts + 1, &A.nd));
    GH_TRY(ctx->reserve(B_GICP_MAHAL, (size_t)npts * 6 + 6, &A.mahal));
    GH_TRY(ctx->reserve(B_ICP_PEND, (size_t)npts + 4, &A.pend));
    GH_TRY(ctx->reserve(B_ICP_PART, (size_t)np * NBLK * NPART, &A.part));
    GH_TRY(ctx->reserve(B_RF_MISC, (size_t)np * 3, &misc));
    A.pair = dd;
    A.pendc = misc;
    A.ovl = misc + np;
    A.flag = reinterpret_cast<unsigned char*>(misc + 2 * (size_t)np);
    hipEvent_t kt = ctx->kt_begin(KT_GICP_CLOUDS);
    GH_TRY(ctx->upload_table(hd.data(), (size_t)np * sizeof(GicpPair), dd));
    GH_TRY(ctx->upload_table(hs.data(), (size_t)np * sizeof(GicpState), A.st));
    // the first search serves the overlap gate and the first iteration: both see the source under the initial transformation_
    GH_TRY(move_and_search(ctx, A, np, max_gs, 0));
    if (P->use_trimmed) {  // common_reg.cpp:240-246
      GH_HIP(hipMemsetAsync(A.ovl, 0, (size_t)np * sizeof(unsigned), s));
      hipLaunchKernelGGL(k_gb_overlap, dim3(max_gs, np), dim3(256), 0, s, A, P->thre_dis * P->thre_dis);
      hovl.assign((size_t)np, 0u);
      GH_HIP(hipMemcpyAsync(hovl.data(), A.ovl, (size_t)np * sizeof(unsigned), hipMemcpyDeviceToHost, s));
      GH_HIP(hipStreamSynchronize(s));
      running = 0;
      for (int q = 0; q < np; q++) {
        GicpState& st = hs[q];
        if (st.refused) continue;
        const float ratio = (float)((0.01 + (int)hovl[q]) / (double)hd[q].ns);  // common_reg.cpp:313
        out[b0 + q].stats.overlap = ratio;
        if (ratio < P->min_overlap) { st.refused = 1; continue; }  // "This registration would not be done"
        running++;
      }
      GH_TRY(ctx->upload_table(hs.data(), (size_t)np * sizeof(GicpState), A.st));  // (no kernel has written a state yet)
    }
    unsigned char* pin = reinterpret_cast<unsigned char*>(ctx->pinned);
    static_assert(kRefineMaxChunk <= 4096, "one status byte per pair must fit the pinned scratch");
    bool have_nn = true;
    while (running > 0) {
      if (!have_nn) GH_TRY(move_and_search(ctx, A, np, max_gs, 0));
      have_nn = false;
      hipLaunchKernelGGL(k_gb_mahal, dim3(NBLK, np), dim3(256), 0, s, A);
      hipLaunchKernelGGL(k_gb_prep, dim3(np), dim3(64), 0, s, A);
      for (int k = 0; k < P->max_inner_iter; k++) {
        hipLaunchKernelGGL(k_gb_acc, dim3(NBLK, np), dim3(256), 0, s, A);
        hipLaunchKernelGGL(k_gb_solve, dim3(np), dim3(64), 0, s, A);
      }
      hipLaunchKernelGGL(k_gb_outer, dim3(cdiv(np, 64)), dim3(64), 0, s, A, np);
      GH_HIP(hipGetLastError());
      GH_HIP(hipMemcpyAsync(pin, A.flag, (size_t)np, hipMemcpyDeviceToHost, s));
      GH_HIP(hipStreamSynchronize(s));
      running = 0;
      for (int q = 0; q < np; q++) running += pin[q] ? 0 : 1;
    }
    // output = the final transformation_ * input, then getFitnessScore() on it
    GH_TRY(move_and_search(ctx, A, np, max_gs, 1));
    hipLaunchKernelGGL(k_gb_sum, dim3(NBLK, np), dim3(256), 0, s, A);
    hipLaunchKernelGGL(k_gb_fitness, dim3(cdiv(np, 64)), dim3(64), 0, s, A, np);
    GH_HIP(hipGetLastError());
    GH_HIP(hipMemcpyAsync(hs.data(), A.st, (size_t)np * sizeof(GicpState), hipMemcpyDeviceToHost, s));
    ctx->kt_end(KT_GICP_CLOUDS, kt);
    GH_HIP(hipStreamSynchronize(s));
    for (int q = 0; q < np; q++) {
      const GicpState& st = hs[q];
      if (st.refused) continue;  // refused (or empty): T = the rounded init, filled above
      ghicp_gicp_result& R = out[b0 + q];
      R.stats.done = 1;
      R.stats.iterations = st.iterations;
      R.stats.converged = st.converged;
      R.stats.reason = st.reason;
      R.stats.correspondences = st.count;
      R.stats.mse = st.mse;
      R.stats.fitness = st.fit_sum / (double)hd[q].ns;
      memcpy(R.T, st.T, sizeof(st.T));
    }
  }
  return GHICP_OK;
}
