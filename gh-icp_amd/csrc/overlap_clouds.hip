// CRegistration::calOverlap (reference src/common_reg.cpp:294-317) for MANY pairs of cached clouds in one launch: which of these pairs overlap
// at all under these poses?
//   ghicp_cloud_prepare_overlap  once per cloud: the search grid of cell thre_dis over its down-sampled points, kept in buffers of the handle
//                                (ghicp_cal_overlap rebuilds it over its second cloud for every pair)
//   ghicp_overlap_clouds         per chunk of pairs ONE launch of k_ov_pairs on a 1-D grid: the concatenation of cdiv(ns, 256) blocks per pair,
//                                no block spans two pairs, a pair with an empty side owns no block.  A block finds its pair by binary search in
//                                the chunk's table of first-block indices (overlap_plan.h); the pair index is uniform over the block, so the
//                                descriptor reads are scalar loads.  A thread loads its source point (16 B, coalesced), moves it by the pair's
//                                float pose (xf_point: the expression of k_transform_f32) and runs the body of k_overlap (overlap_hit,
//                                icp_dev.h).  The moved source is never stored: compulsory traffic is 16 B per source point plus the target
//                                cells touched.  A hopeless pair costs its 16 B per point: every query fails the padded-grid test.
//   ghicp_overlap_matrix         all ordered pairs of n clouds under cloud->world poses: the pose products on the host, one ghicp_overlap_clouds
// The counts are integers (one atomic per block): no float atomics, nothing depends on the block order.  hits and ratio of a pair are those
// of ghicp_transform_cloud_f32 + ghicp_cal_overlap on its down-sampled clouds, bit for bit.  The host reads one unsigned per pair.
#include "cloud.h"
#include "icp_dev.h"
#include "overlap_plan.h"

#include <algorithm>

namespace {

using namespace icpdev;

struct OvPair {
  NnGrid G;           // the target's grid of cell thre_dis (buffers of its handle)
  const float4* src;  // the source's down-sampled points
  int ns, pad_;
  float init[16];     // float(Rt)
};

__global__ __launch_bounds__(256) void k_ov_pairs(const OvPair* __restrict__ pair, const int* __restrict__ first, int np, float r2,
                                                  unsigned* __restrict__ count) {
  const int q = gh_ov_pair_of_block(first, np, (int)blockIdx.x);
  const OvPair& D = pair[q];
  const int i = ((int)blockIdx.x - first[q]) * kOvBlock + (int)threadIdx.x;
  bool hit = false;
  if (i < D.ns) {
    const float4 S = D.src[i];
    const float4 P = xf_point(D.init, S.x, S.y, S.z);
    hit = overlap_hit(D.G, P.x, P.y, P.z, r2);
  }
  block_count_add(hit, &count[q]);
}

const GridSlots kSlotsOv = {B_GRID2_KEYS, B_GRID2_KEYS2, B_GRID2_VALS, B_GRID2_VALS2, B_GRID2_START, B_GRID2_PTS};  // those of ghicp_cal_overlap

// what both entry points ask of a handle; `what` names it in the message
int check_handle(ghicp_ctx* ctx, const char* fn, const ghicp_cloud* c, bool as_target, float thre_dis, const char* what, int index) {
  if (!c || !c->ctx || c->ctx->device != ctx->device) return ctx->fail(GHICP_ERR_ARG, "%s: %s %d is NULL or a handle of another device", fn, what, index);
  if (!c->ds.p) return ctx->fail(GHICP_ERR_ARG, "%s: %s %d was rebuilt from stored features and holds no points", fn, what, index);
  if (as_target && !(c->ov_ready && c->ov_thre == thre_dis))
    return ctx->fail(GHICP_ERR_ARG, "%s: %s %d holds no search grid for thre_dis = %g (ghicp_cloud_prepare_overlap)", fn, what, index, (double)thre_dis);
  return GHICP_OK;
}

}  // namespace

extern "C" int ghicp_cloud_prepare_overlap(ghicp_cloud* c, float thre_dis) {
  if (!c || !c->ctx) return GHICP_ERR_ARG;
  ghicp_ctx* ctx = c->ctx;
  GH_ENTER(ctx);
  GH_ARG(thre_dis > 0.f);
  if (!c->ds.p) return ctx->fail(GHICP_ERR_ARG, "ghicp_cloud_prepare_overlap: this handle was rebuilt from stored features and holds no points");
  if (c->ov_ready && c->ov_thre == thre_dis) return GHICP_OK;
  hipStream_t s = ctx->stream;
  c->ov_invalidate();  // until everything below is in place
  memset(&c->ov_grid, 0, sizeof(GridDesc));
  if (c->m > 0) {
    DeviceGrid g;
    GH_TRY(gh_grid_build(ctx, reinterpret_cast<const float*>(c->ds.p), c->m, 4, thre_dis, kSlotsOv, &g));
    // out of the context's grid buffers into the handle's own
    GH_HIP(c->ov_pts.reserve((size_t)c->m * sizeof(float4)));
    GH_HIP(c->ov_start.reserve(((size_t)g.d.ncell + 1) * sizeof(unsigned)));
    GH_HIP(hipMemcpyAsync(c->ov_pts.p, g.pts, (size_t)c->m * sizeof(float4), hipMemcpyDeviceToDevice, s));
    GH_HIP(hipMemcpyAsync(c->ov_start.p, g.start, ((size_t)g.d.ncell + 1) * sizeof(unsigned), hipMemcpyDeviceToDevice, s));
    c->ov_grid = g.d;
  }
  GH_HIP(hipStreamSynchronize(s));  // afterwards the handle may serve any context of the device
  c->ov_thre = thre_dis;
  c->ov_ready = true;
  return GHICP_OK;
}

extern "C" int ghicp_overlap_clouds(ghicp_ctx* ctx, float thre_dis, int32_t n_pairs, const ghicp_cloud* const* S, const ghicp_cloud* const* T,
                                    const double* Rt, int32_t max_concurrent, ghicp_overlap_result* out) {
  GH_ENTER(ctx);
  GH_ARG(n_pairs >= 0 && max_concurrent >= 0 && (n_pairs == 0 || (S != nullptr && T != nullptr && out != nullptr)));
  GH_ARG(thre_dis > 0.f);
  // every pair is checked before anything is written or launched
  std::vector<int64_t> ns_all((size_t)n_pairs);
  for (int i = 0; i < n_pairs; i++) {
    GH_TRY(check_handle(ctx, "ghicp_overlap_clouds", S[i], false, thre_dis, "the source of pair", i));
    GH_TRY(check_handle(ctx, "ghicp_overlap_clouds", T[i], true, thre_dis, "the target of pair", i));
    ns_all[i] = S[i]->m > 0 && T[i]->m > 0 ? S[i]->m : 0;  // a pair with an empty side launches nothing
  }
  if (n_pairs == 0) return GHICP_OK;
  hipStream_t s = ctx->stream;
  const float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const std::vector<OvChunk> plan = gh_overlap_plan(n_pairs, ns_all.data(), max_concurrent);
  // a chunk's table: its descriptors, then its first-block indices
  auto desc_bytes = [](int np) { return (size_t)np * sizeof(OvPair); };
  size_t table_max = 0;
  for (const OvChunk& ch : plan) table_max = std::max(table_max, desc_bytes(ch.p1 - ch.p0) + ch.first.size() * sizeof(int));
  char* dtab;
  unsigned* dcount;
  GH_TRY(ctx->reserve(B_RF_DESC, table_max, &dtab));
  GH_TRY(ctx->reserve(B_RF_MISC, (size_t)n_pairs, &dcount));
  GH_HIP(hipMemsetAsync(dcount, 0, (size_t)n_pairs * sizeof(unsigned), s));
  std::vector<char> htab;
  for (const OvChunk& ch : plan) {
    const int np = ch.p1 - ch.p0, blocks = ch.first.back();
    if (blocks == 0) continue;
    htab.assign(desc_bytes(np) + ch.first.size() * sizeof(int), 0);
    OvPair* hd = reinterpret_cast<OvPair*>(htab.data());
    for (int q = 0; q < np; q++) {
      const int p = ch.p0 + q;
      if (ns_all[p] == 0) continue;
      const ghicp_cloud *a = S[p], *b = T[p];
      OvPair& D = hd[q];
      D.G = NnGrid{b->ov_grid, b->ov_pts.as<float4>(), b->ov_start.as<unsigned>(), 1.0f / b->ov_grid.inv};
      D.src = a->ds.as<float4>();
      D.ns = (int)a->m;
      for (int e = 0; e < 16; e++) D.init[e] = Rt ? (float)Rt[(size_t)p * 16 + e] : I16[e];
    }
    memcpy(htab.data() + desc_bytes(np), ch.first.data(), ch.first.size() * sizeof(int));
    GH_TRY(ctx->upload_table(htab.data(), htab.size(), dtab));
    hipLaunchKernelGGL(k_ov_pairs, dim3((unsigned)blocks), dim3(kOvBlock), 0, s, reinterpret_cast<const OvPair*>(dtab),
                       reinterpret_cast<const int*>(dtab + desc_bytes(np)), np, thre_dis * thre_dis, dcount + ch.p0);
    GH_HIP(hipGetLastError());
  }
  std::vector<unsigned> hits((size_t)n_pairs, 0u);
  GH_HIP(hipMemcpyAsync(hits.data(), dcount, (size_t)n_pairs * sizeof(unsigned), hipMemcpyDeviceToHost, s));
  GH_HIP(hipStreamSynchronize(s));
  for (int p = 0; p < n_pairs; p++) {
    ghicp_overlap_result& R = out[p];
    memset(&R, 0, sizeof(R));
    R.hits = (int64_t)hits[p];
    R.n = S[p]->m;
    R.ratio = R.n > 0 ? (float)((0.01 + (int)hits[p]) / (double)R.n) : 0.f;  // common_reg.cpp:313
  }
  return GHICP_OK;
}

extern "C" int ghicp_overlap_matrix(ghicp_ctx* ctx, float thre_dis, int32_t n_clouds, const ghicp_cloud* const* clouds, const double* poses, float* out) {
  GH_ENTER(ctx);
  GH_ARG(n_clouds >= 0 && n_clouds <= 32768 && (n_clouds == 0 || (clouds != nullptr && out != nullptr)));
  GH_ARG(thre_dis > 0.f);
  for (int i = 0; i < n_clouds; i++) GH_TRY(check_handle(ctx, "ghicp_overlap_matrix", clouds[i], true, thre_dis, "cloud", i));  // every handle is a target
  if (n_clouds == 0) return GHICP_OK;
  const size_t np = (size_t)n_clouds * (size_t)(n_clouds - 1);
  std::vector<const ghicp_cloud*> S(np), T(np);
  std::vector<double> Rt(poses ? np * 16 : 0);
  size_t p = 0;
  for (int i = 0; i < n_clouds; i++)
    for (int j = 0; j < n_clouds; j++) {
      if (i == j) continue;
      S[p] = clouds[i];
      T[p] = clouds[j];
      if (poses) {  // inv(P_j) * P_i of two rigid poses: R_j^T R_i and R_j^T (t_i - t_j), every sum of three terms added left to right
        const double *Pi = poses + (size_t)i * 16, *Pj = poses + (size_t)j * 16;
        double* M = &Rt[p * 16];
        const double d[3] = {Pi[3] - Pj[3], Pi[7] - Pj[7], Pi[11] - Pj[11]};
        for (int r = 0; r < 3; r++) {
          for (int c = 0; c < 3; c++) M[r * 4 + c] = (Pj[0 * 4 + r] * Pi[0 * 4 + c] + Pj[1 * 4 + r] * Pi[1 * 4 + c]) + Pj[2 * 4 + r] * Pi[2 * 4 + c];
          M[r * 4 + 3] = (Pj[0 * 4 + r] * d[0] + Pj[1 * 4 + r] * d[1]) + Pj[2 * 4 + r] * d[2];
        }
        M[12] = M[13] = M[14] = 0.0;
        M[15] = 1.0;
      }
      p++;
    }
  std::vector<ghicp_overlap_result> res(np);
  if (np > 0) GH_TRY(ghicp_overlap_clouds(ctx, thre_dis, (int32_t)np, S.data(), T.data(), poses ? Rt.data() : nullptr, 0, res.data()));
  p = 0;
  for (int i = 0; i < n_clouds; i++)
    for (int j = 0; j < n_clouds; j++) out[(size_t)i * n_clouds + j] = i == j ? 1.0f : res[p++].ratio;
  return GHICP_OK;
}
