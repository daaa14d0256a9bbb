// Fine registration on gfx950: CRegistration<PointT>::icp_reg / ptplicp_reg / calOverlap / transformcloud / invTransform
// (reference include/common_reg.h:26-110, src/common_reg.cpp:45-107, 122-199, 294-317, 325-370).  The reference hands the
// loop to PCL (IterativeClosestPoint[WithNormals], CorrespondenceRejectorTrimmed, KdTreeFLANN); here it is
//   k_nn_fine / k_nn_coarse  exact 1-NN of every (transformed) source point in the target: thread-per-query ring search
//                            on a fine uniform grid, the unresolved tail (queries far from the target) handed to a
//                            wave-per-query search on an 8x coarser grid.  float L2, ties -> lower index.
//   k_sel_pass (radix select) the trimmed rejector (keep the floor(overlap * count) smallest by (d^2, source index))
//   k_acc_means / k_acc_cov  float Umeyama sums in f64 (N2), per-block partials reduced in a fixed order
//   k_acc_plane              point-to-plane LLS normal equations (6x6, f64 sums of float terms)
//   k_icp_step               the closed-form solve + pcl DefaultConvergenceCriteria, one thread
//   k_apply                  transformation_ applied to the working copy of the source
// One 64-byte status record per iteration is the only device->host traffic.  HBM-bound: per iteration the compulsory
// traffic is 16 B in + 16 B out per source point plus the target cells each query touches.
#include "icp_dev.h"

int gh_knn_normals_dev(ghicp_ctx* ctx, const float* xyz, long long m, int stride, int k, float* normals);

namespace {

using namespace icpdev;

// ------------------------------------------------------------------------------------------------ 1-NN search (bodies: icp_dev.h)
__global__ __launch_bounds__(256) void k_nn_fine(NnGrid G, const float4* __restrict__ q, int nq, int* __restrict__ nn, float* __restrict__ nd,
                                                 unsigned* __restrict__ pend_list, unsigned* __restrict__ pend_count) {
  nn_fine_body(G, q, nq, blockIdx.x * 256 + threadIdx.x, nn, nd, pend_list, pend_count);
}

__global__ __launch_bounds__(256) void k_nn_coarse(NnGrid G, const float4* __restrict__ q, const unsigned* __restrict__ pend_list,
                                                   const unsigned* __restrict__ pend_count, int* __restrict__ nn, float* __restrict__ nd) {
  nn_coarse_body(G, q, pend_list, *pend_count, blockIdx.x * 4u + (threadIdx.x >> 6), gridDim.x * 4u, nn, nd);
}

__global__ __launch_bounds__(256) void k_count_occupied(const unsigned* __restrict__ keys, unsigned n, unsigned* __restrict__ out) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const bool first = i < n && (i == 0 || keys[i] != keys[i - 1]);
  block_count_add(first, out);
}

__global__ __launch_bounds__(256) void k_pack4(const float* __restrict__ xyz, long long n, int stride, float4* __restrict__ out) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i < n) out[i] = make_float4(xyz[i * stride], xyz[i * stride + 1], xyz[i * stride + 2], 0.f);
}

__global__ __launch_bounds__(256) void k_gather_query(const float4* __restrict__ tgt, const int* __restrict__ nn, int n, float4* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = tgt[max(nn[i], 0)];
}

__global__ __launch_bounds__(256) void k_reciprocal(const int* __restrict__ back, int n, int* __restrict__ nn) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && back[i] != i) nn[i] = -1;
}

// ------------------------------------------------------------------------------------------------ overlap
__global__ __launch_bounds__(256) void k_overlap(NnGrid G, const float* __restrict__ xyz, long long n, int stride, float r2, unsigned* __restrict__ count) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  bool hit = false;
  if (i < n) {
    const float px = xyz[i * stride], py = xyz[i * stride + 1], pz = xyz[i * stride + 2];
    hit = overlap_hit(G, px, py, pz, r2);  // icp_dev.h
  }
  block_count_add(hit, count);
}

// ------------------------------------------------------------------------------------------------ correspondences
__global__ __launch_bounds__(256) void k_corr_count(const int* __restrict__ nn, int n, IcpState* __restrict__ st) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  block_count_add(i < n && nn[i] >= 0, &st->count);
}

__global__ void k_icp_prep(IcpState* st) { icp_prep_body(st); }

__global__ __launch_bounds__(256) void k_sel_pass(int pass, const int* __restrict__ nn, const float* __restrict__ nd, int n, IcpState* __restrict__ st,
                                                  unsigned* __restrict__ hist) {
  sel_pass_body(pass, nn, nd, n, st, hist, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(256) void k_sel_final(IcpState* __restrict__ st, const unsigned* __restrict__ hist) { sel_final_body(st, hist); }

__global__ __launch_bounds__(256) void k_acc_means(CorrView V, const IcpState* __restrict__ st, double* __restrict__ part) { acc_means_body(V, st, part, blockIdx.x); }

__global__ __launch_bounds__(64) void k_icp_means(IcpState* st, const double* __restrict__ part) { icp_means_body(st, part); }

__global__ __launch_bounds__(256) void k_acc_cov(CorrView V, const IcpState* __restrict__ st, double* __restrict__ part) { acc_cov_body(V, st, part, blockIdx.x); }

__global__ __launch_bounds__(256) void k_acc_plane(CorrView V, const float* __restrict__ tnrm, const IcpState* __restrict__ st, double* __restrict__ part) {
  acc_plane_body(V, tnrm, st, part, blockIdx.x);
}

__global__ __launch_bounds__(64) void k_icp_step(IcpState* st, const double* __restrict__ part) { icp_step_body(st, part); }

__global__ __launch_bounds__(256) void k_apply(float4* __restrict__ cur, int n, const IcpState* __restrict__ st) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (st->reason == GHICP_ICP_NO_CORRESPONDENCES) return;
  const float4 P = cur[i];
  cur[i] = xf_point(st->T, P.x, P.y, P.z);
}

struct M16 { float m[16]; };
__global__ __launch_bounds__(256) void k_transform_f32(const float* __restrict__ xyz, long long n, int stride, M16 M, float* __restrict__ out3,
                                                       float4* __restrict__ out4) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const float x = xyz[i * stride], y = xyz[i * stride + 1], z = xyz[i * stride + 2];
  const float ox = ((M.m[0] * x + M.m[1] * y) + M.m[2] * z) + M.m[3];
  const float oy = ((M.m[4] * x + M.m[5] * y) + M.m[6] * z) + M.m[7];
  const float oz = ((M.m[8] * x + M.m[9] * y) + M.m[10] * z) + M.m[11];
  if (out3) { out3[i * 3] = ox; out3[i * 3 + 1] = oy; out3[i * 3 + 2] = oz; }
  if (out4) out4[i] = make_float4(ox, oy, oz, 0.f);
}

__global__ __launch_bounds__(256) void k_sum_f32(const float* __restrict__ v, int n, double* __restrict__ part) { sum_f32_body(v, n, part, blockIdx.x); }

// ------------------------------------------------------------------------------------------------ host side
const GridSlots kSlotsTF = {B_GRID_KEYS, B_GRID_KEYS2, B_GRID_VALS, B_GRID_VALS2, B_GRID_START, B_GRID_PTS};
const GridSlots kSlotsTC = {B_ICP_TC_KEYS, B_ICP_TC_KEYS2, B_ICP_TC_VALS, B_ICP_TC_VALS2, B_ICP_TC_START, B_ICP_TC_PTS};
const GridSlots kSlotsSF = {B_GRID2_KEYS, B_GRID2_KEYS2, B_GRID2_VALS, B_GRID2_VALS2, B_GRID2_START, B_GRID2_PTS};
const GridSlots kSlotsSC = {B_ICP_SC_KEYS, B_ICP_SC_KEYS2, B_ICP_SC_VALS, B_ICP_SC_VALS2, B_ICP_SC_START, B_ICP_SC_PTS};

NnGrid as_nn(const DeviceGrid& g) { return NnGrid{g.d, g.pts, g.start, 1.0f / g.d.inv}; }

// Builds the fine + coarse grids over xyz.  cell <= 0: pick the cell from the data -- start from a volume guess and halve
// it while the occupied cells hold more than ~8 points on average (surface scans fill a small share of their bounding box).
int build_index(ghicp_ctx* ctx, const float* xyz, long long n, int stride, float cell, const GridSlots& sf, const GridSlots& sc, NnIndex* out,
                float* cell_used) {
  hipStream_t s = ctx->stream;
  DeviceGrid gf, gc;
  if (cell > 0.f) {
    GH_TRY(gh_grid_build(ctx, xyz, n, stride, cell, sf, &gf));
  } else {
    float mm[6];
    GH_TRY(gh_bbox_dev(ctx, xyz, n, stride, mm));
    const double vol = fmax(1e-9, (double)(mm[3] - mm[0] + 1e-3) * (mm[4] - mm[1] + 1e-3) * (mm[5] - mm[2] + 1e-3));
    cell = fmaxf((float)cbrt(vol / (double)n * 8.0), 0.02f);
    unsigned* cnt;
    GH_TRY(ctx->reserve(B_ICP_PEND, (size_t)n + 4, &cnt));
    for (int attempt = 0;; attempt++) {
      GH_TRY(gh_grid_build(ctx, xyz, n, stride, cell, sf, &gf));
      if (attempt >= 5) break;
      const double nc_next = (double)gf.d.dim[0] * gf.d.dim[1] * gf.d.dim[2] * 8.0;
      if (nc_next > (double)(1u << 26) || 1.0f / gf.d.inv > cell * 1.01f) break;  // next halving would not fit / was already coarsened
      GH_HIP(hipMemsetAsync(cnt, 0, 4, s));
      hipLaunchKernelGGL(k_count_occupied, dim3(cdiv(n, 256)), dim3(256), 0, s, gf.keys, (unsigned)n, cnt);
      unsigned occ = 0;
      GH_HIP(hipMemcpyAsync(&occ, cnt, 4, hipMemcpyDeviceToHost, s));
      GH_HIP(hipStreamSynchronize(s));
      if (occ == 0 || (double)n / occ <= 8.0) break;
      cell *= 0.5f;
    }
  }
  const float cf = 1.0f / gf.d.inv;
  GH_TRY(gh_grid_build(ctx, xyz, n, stride, cf * 8.0f, sc, &gc));
  out->fine = as_nn(gf);
  out->coarse = as_nn(gc);
  if (cell_used) *cell_used = cf;
  return GHICP_OK;
}

int nn_search(ghicp_ctx* ctx, const NnIndex& X, const float4* q, int nq, int* nn, float* nd) {
  if (nq <= 0) return GHICP_OK;
  hipStream_t s = ctx->stream;
  unsigned* pend;
  GH_TRY(ctx->reserve(B_ICP_PEND, (size_t)nq + 4, &pend));
  GH_HIP(hipMemsetAsync(pend, 0, 4, s));
  hipLaunchKernelGGL(k_nn_fine, dim3(cdiv(nq, 256)), dim3(256), 0, s, X.fine, q, nq, nn, nd, pend + 1, pend);
  hipLaunchKernelGGL(k_nn_coarse, dim3(min(cdiv(nq, 4), 4096)), dim3(256), 0, s, X.coarse, q, pend + 1, pend, nn, nd);
  GH_HIP(hipGetLastError());
  return GHICP_OK;
}

int overlap_dev(ghicp_ctx* ctx, const float* d1, long long n1, int s1, const float* d2, long long n2, int s2, float thre_dis, float* ratio) {
  if (n1 <= 0) { *ratio = 0.f; return GHICP_OK; }
  unsigned cnt_h = 0;
  if (n2 > 0) {
    DeviceGrid g;
    GH_TRY(gh_grid_build(ctx, d2, n2, s2, thre_dis, kSlotsSF, &g));
    unsigned* cnt;
    GH_TRY(ctx->reserve(B_ICP_STATE, 64, &cnt));
    GH_HIP(hipMemsetAsync(cnt, 0, 4, ctx->stream));
    hipLaunchKernelGGL(k_overlap, dim3(cdiv(n1, 256)), dim3(256), 0, ctx->stream, as_nn(g), d1, n1, s1, thre_dis * thre_dis, cnt);
    GH_HIP(hipMemcpyAsync(&cnt_h, cnt, 4, hipMemcpyDeviceToHost, ctx->stream));
    GH_HIP(hipStreamSynchronize(ctx->stream));
  }
  *ratio = (float)((0.01 + (int)cnt_h) / (double)n1);  // common_reg.cpp:313
  return GHICP_OK;
}

// ------------------------------------------------------------------------------------------------ generalized ICP
// CRegistration::gicp_reg (common_reg.cpp:216-284) = pcl::GeneralizedIterativeClosestPoint as recalled in ghicp_c.h, with the inner
// solver of DESIGN.md N8.  Per outer iteration: k_gicp_apply, the 1-NN search, k_gicp_mahal, k_gicp_prep, max_inner_iter x
// (k_gicp_acc, k_gicp_solve), k_gicp_outer, one status read.  The inner steps after the stop flag are no-ops.
// the bodies are in icp_dev.h, shared with the batched loop over cached clouds (refine_gicp.hip)
__global__ __launch_bounds__(256) void k_gicp_apply(const float4* __restrict__ src, int n, const GicpState* __restrict__ st, float4* __restrict__ cur) {
  gicp_apply_body(src, n, blockIdx.x * 256 + threadIdx.x, st, cur);
}

__global__ __launch_bounds__(256) void k_gicp_mahal(int* __restrict__ nn, const float* __restrict__ nd, int ns, const double* __restrict__ covS,
                                                    const double* __restrict__ covT, const GicpState* __restrict__ st, double* __restrict__ mahal,
                                                    double* __restrict__ part) {
  gicp_mahal_body(nn, nd, ns, covS, covT, st, mahal, part, blockIdx.x);
}

__global__ __launch_bounds__(64) void k_gicp_prep(GicpState* st, const double* __restrict__ part) { gicp_prep_body(st, part); }

__global__ __launch_bounds__(256) void k_gicp_acc(const float4* __restrict__ src, const float4* __restrict__ tgt, const int* __restrict__ nn, int ns,
                                                  const double* __restrict__ mahal, const GicpState* __restrict__ st, double* __restrict__ part) {
  gicp_acc_body(src, tgt, nn, ns, mahal, st, part, blockIdx.x);
}

__global__ __launch_bounds__(64) void k_gicp_solve(GicpState* st, const double* __restrict__ part) { gicp_solve_body(st, part); }

__global__ void k_gicp_outer(GicpState* st) { gicp_outer_body(st); }

// The trimmed loop (ghicp_gicp_trimmed_from): between the search and k_gicp_prep, k_gicp_reject, k_gicp_trim_prep, the radix select of the ICP
// path over the survivors (the bodies of k_sel_pass / k_sel_final on the GicpSel record) and k_gicp_mahal_trim in the place of k_gicp_mahal.
__global__ __launch_bounds__(256) void k_gicp_reject(int* __restrict__ nn, const float* __restrict__ nd, int ns, const GicpState* __restrict__ st,
                                                     GicpSel* __restrict__ sel) {
  gicp_reject_body(nn, nd, ns, blockIdx.x * 256 + threadIdx.x, st, sel);
}

__global__ void k_gicp_trim_prep(const GicpState* __restrict__ st, GicpSel* __restrict__ sel) { gicp_trim_prep_body(st, sel); }

__global__ __launch_bounds__(256) void k_gicp_sel_pass(int pass, const int* __restrict__ nn, const float* __restrict__ nd, int n, GicpSel* __restrict__ sel,
                                                       unsigned* __restrict__ hist) {
  sel_pass_body(pass, nn, nd, n, sel, hist, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(256) void k_gicp_sel_final(GicpSel* __restrict__ sel, const unsigned* __restrict__ hist) { sel_final_body(sel, hist); }

__global__ __launch_bounds__(256) void k_gicp_mahal_trim(int* __restrict__ nn, const float* __restrict__ nd, int ns, const double* __restrict__ covS,
                                                         const double* __restrict__ covT, const GicpState* __restrict__ st,
                                                         const GicpSel* __restrict__ sel, double* __restrict__ mahal, double* __restrict__ part) {
  gicp_mahal_trim_body(nn, nd, ns, covS, covT, st, sel, mahal, part, blockIdx.x);
}

}  // namespace

int gh_icp_build_index(ghicp_ctx* ctx, const float* xyz, long long n, int stride, icpdev::NnIndex* out) {
  return build_index(ctx, xyz, n, stride, 0.f, kSlotsTF, kSlotsTC, out, nullptr);
}

extern "C" void ghicp_icp_params_default(ghicp_icp_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->max_iter = 50;
  p->metric = GHICP_ICP_POINT_TO_POINT;
  p->thre_dis = 0.5f;
  p->min_overlap = 0.1f;
  p->covariance_k = 15;
  p->transformation_epsilon = 1e-8;
  p->euclidean_fitness_epsilon = 1e-5;
}

extern "C" void ghicp_inv_transform(const float* T, float* inv) {
  float t[16];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) t[r * 4 + c] = T[c * 4 + r];
  t[3] = -T[3]; t[7] = -T[7]; t[11] = -T[11];
  t[12] = t[13] = t[14] = 0.f;
  t[15] = 1.f;
  memcpy(inv, t, sizeof(t));
}

extern "C" int ghicp_cal_overlap(ghicp_ctx* ctx, const float* xyz1, int64_t n1, int stride1, const float* xyz2, int64_t n2, int stride2,
                                 float thre_dis, float* ratio) {
  GH_ENTER(ctx);
  GH_ARG(n1 >= 0 && n2 >= 0 && n1 < (1ll << 31) - 2 && n2 < (1ll << 31) - 2 && stride1 >= 3 && stride2 >= 3 && thre_dis > 0.f && ratio != nullptr);
  Stager sg(ctx);
  const float *d1, *d2;
  GH_TRY(sg.in_cloud(xyz1, (size_t)n1 * stride1, &d1));
  GH_TRY(sg.in_cloud(xyz2, (size_t)n2 * stride2, &d2));
  return overlap_dev(ctx, d1, n1, stride1, d2, n2, stride2, thre_dis, ratio);
}

extern "C" int ghicp_transform_cloud_f32(ghicp_ctx* ctx, const float* xyz, int64_t n, int stride, const float* T16, float* out) {
  GH_ENTER(ctx);
  GH_ARG(n >= 0 && stride >= 3 && T16 != nullptr);
  Stager sg(ctx);
  const float* d;
  float* o;
  GH_TRY(sg.in_cloud(xyz, (size_t)n * stride, &d));
  GH_TRY(sg.out(out, (size_t)n * 3, &o));
  if (n > 0) {
    M16 M;
    memcpy(M.m, T16, sizeof(M.m));
    hipLaunchKernelGGL(k_transform_f32, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, d, (long long)n, stride, M, o, (float4*)nullptr);
    GH_HIP(hipGetLastError());
  }
  return sg.finish();
}

extern "C" int ghicp_knn_normals(ghicp_ctx* ctx, const float* xyz, int64_t n, int stride, int k, float* normals) {
  GH_ENTER(ctx);
  GH_ARG(n >= 0 && n < (1ll << 31) - 2 && stride >= 3 && normals != nullptr);
  Stager sg(ctx);
  const float* d;
  float* o;
  GH_TRY(sg.in_cloud(xyz, (size_t)n * stride, &d));
  GH_TRY(sg.out(normals, (size_t)n * 3, &o));
  GH_TRY(gh_knn_normals_dev(ctx, d, n, stride, k, o));
  return sg.finish();
}

extern "C" int ghicp_nn_search(ghicp_ctx* ctx, const float* query, int64_t nq, int strideQ, const float* xyzT, int64_t nt, int strideT,
                               int32_t* idx, float* d2) {
  GH_ENTER(ctx);
  GH_ARG(nq >= 0 && nt > 0 && nq < (1ll << 31) - 2 && nt < (1ll << 31) - 2 && strideQ >= 3 && strideT >= 3);
  Stager sg(ctx);
  const float *dq, *dt;
  int32_t* di;
  float* dd;
  GH_TRY(sg.in(query, (size_t)nq * strideQ, &dq));
  GH_TRY(sg.in_cloud(xyzT, (size_t)nt * strideT, &dt));
  GH_TRY(sg.out(idx, (size_t)nq, &di));
  GH_TRY(sg.out(d2, (size_t)nq, &dd));
  if (nq > 0) {
    NnIndex X;
    GH_TRY(build_index(ctx, dt, nt, strideT, 0.f, kSlotsTF, kSlotsTC, &X, nullptr));
    float4* q4;
    GH_TRY(ctx->reserve(B_ICP_Q, (size_t)nq + 1, &q4));
    hipLaunchKernelGGL(k_pack4, dim3(cdiv(nq, 256)), dim3(256), 0, ctx->stream, dq, (long long)nq, strideQ, q4);
    GH_TRY(nn_search(ctx, X, q4, (int)nq, di, dd));
  }
  return sg.finish();
}

extern "C" int ghicp_icp(ghicp_ctx* ctx, const float* xyzS, int64_t ns, int strideS, const float* xyzT, int64_t nt, int strideT,
                         const ghicp_icp_params* P, float* T16, float* transformed, ghicp_icp_stats* stats) {
  GH_ENTER(ctx);
  GH_ARG(P != nullptr && T16 != nullptr && stats != nullptr && ns >= 0 && nt >= 0 && ns < (1ll << 31) - 2 && nt < (1ll << 31) - 2 && strideS >= 3 &&
         strideT >= 3);
  GH_ARG(P->metric == GHICP_ICP_POINT_TO_POINT || P->metric == GHICP_ICP_POINT_TO_PLANE);
  hipStream_t s = ctx->stream;
  memset(stats, 0, sizeof(*stats));
  Stager sg(ctx);
  const float *dS, *dT;
  float* dOut;
  GH_TRY(sg.in_cloud(xyzS, (size_t)ns * strideS, &dS));
  GH_TRY(sg.in_cloud(xyzT, (size_t)nt * strideT, &dT));
  GH_TRY(sg.out(transformed, (size_t)ns * 3, &dOut));

  float ratio = 1.0f;
  int trimmed = 0;
  if (P->use_trimmed) {  // common_reg.cpp:64-74
    GH_ARG(P->thre_dis > 0.f);
    GH_TRY(overlap_dev(ctx, dS, ns, strideS, dT, nt, strideT, P->thre_dis, &ratio));
    stats->overlap = ratio;
    if (ratio < P->min_overlap) { sg.outs.clear(); return GHICP_OK; }  // "This registration would not be done"
    trimmed = ratio < 1.0f;
  }
  stats->done = 1;
  const float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  IcpState hst;
  memset(&hst, 0, sizeof(hst));
  memcpy(hst.fin, I16, sizeof(I16));
  memcpy(hst.T, I16, sizeof(I16));
  if (ns == 0 || nt == 0) {
    stats->reason = GHICP_ICP_NO_CORRESPONDENCES;
    memcpy(T16, I16, sizeof(I16));
    if (ns > 0 && dOut) {
      M16 M;
      memcpy(M.m, I16, sizeof(I16));
      hipLaunchKernelGGL(k_transform_f32, dim3(cdiv(ns, 256)), dim3(256), 0, s, dS, (long long)ns, strideS, M, dOut, (float4*)nullptr);
    }
    return sg.finish();
  }

  float4 *cur, *tgt4, *q4 = nullptr;
  int *nn, *nn2 = nullptr;
  float *nd, *nd2 = nullptr, *tnrm = nullptr;
  unsigned* hist = nullptr;
  double* part;
  IcpState* st;
  GH_TRY(ctx->reserve(B_ICP_CUR, (size_t)ns + 1, &cur));
  GH_TRY(ctx->reserve(B_ICP_OUT, (size_t)nt + 1, &tgt4));
  GH_TRY(ctx->reserve(B_ICP_NN, (size_t)ns + 1, &nn));
  GH_TRY(ctx->reserve(B_ICP_ND, (size_t)ns + 1, &nd));
  GH_TRY(ctx->reserve(B_ICP_PART, (size_t)NBLK * NPART, &part));
  GH_TRY(ctx->reserve(B_ICP_STATE, 1, &st));
  if (P->use_reciprocal) {
    GH_TRY(ctx->reserve(B_ICP_Q, (size_t)ns + 1, &q4));
    GH_TRY(ctx->reserve(B_ICP_NN2, (size_t)ns + 1, &nn2));
    GH_TRY(ctx->reserve(B_ICP_ND2, (size_t)ns + 1, &nd2));
  }
  if (trimmed) GH_TRY(ctx->reserve(B_ICP_KEYS, (size_t)6 * SEL_BINS, &hist));
  if (P->metric == GHICP_ICP_POINT_TO_PLANE) {  // common_reg.cpp:146-147 (only the target normals enter the LLS solve)
    GH_TRY(ctx->reserve(B_ICP_TNRM, (size_t)nt * 3 + 3, &tnrm));
    GH_TRY(gh_knn_normals_dev(ctx, dT, nt, strideT, P->covariance_k, tnrm));
  }
  hipLaunchKernelGGL(k_pack4, dim3(cdiv(ns, 256)), dim3(256), 0, s, dS, (long long)ns, strideS, cur);
  hipLaunchKernelGGL(k_pack4, dim3(cdiv(nt, 256)), dim3(256), 0, s, dT, (long long)nt, strideT, tgt4);
  NnIndex XT, XS;
  float cell = 0.f;
  GH_TRY(build_index(ctx, dT, nt, strideT, 0.f, kSlotsTF, kSlotsTC, &XT, &cell));

  hst.prev_mse = 1.7976931348623157e308;
  hst.eps_t = P->transformation_epsilon;
  hst.eps_e = P->euclidean_fitness_epsilon;
  hst.max_iter = P->max_iter;
  hst.trimmed = trimmed;
  hst.metric = P->metric;
  hst.ratio = ratio;
  GH_HIP(hipMemcpyAsync(st, &hst, sizeof(hst), hipMemcpyHostToDevice, s));
  IcpState* pin = reinterpret_cast<IcpState*>(ctx->pinned);
  static_assert(sizeof(IcpState) <= 4096, "status record must fit the pinned scratch");
  const int gS = cdiv(ns, 256);
  const CorrView V = {nn, nd, cur, tgt4, (int)ns};
  const int gSel = min(cdiv(ns, 2048), 512);
  for (;;) {
    GH_TRY(nn_search(ctx, XT, cur, (int)ns, nn, nd));
    if (P->use_reciprocal) {  // determineReciprocalCorrespondences
      GH_TRY(build_index(ctx, reinterpret_cast<const float*>(cur), ns, 4, cell, kSlotsSF, kSlotsSC, &XS, nullptr));
      hipLaunchKernelGGL(k_gather_query, dim3(gS), dim3(256), 0, s, tgt4, nn, (int)ns, q4);
      GH_TRY(nn_search(ctx, XS, q4, (int)ns, nn2, nd2));
      hipLaunchKernelGGL(k_reciprocal, dim3(gS), dim3(256), 0, s, nn2, (int)ns, nn);
    }
    hipLaunchKernelGGL(k_corr_count, dim3(gS), dim3(256), 0, s, nn, (int)ns, st);
    hipLaunchKernelGGL(k_icp_prep, dim3(1), dim3(1), 0, s, st);
    if (trimmed) {
      GH_HIP(hipMemsetAsync(hist, 0, (size_t)6 * SEL_BINS * sizeof(unsigned), s));
      for (int pass = 0; pass < 6; pass++) hipLaunchKernelGGL(k_sel_pass, dim3(gSel), dim3(256), 0, s, pass, nn, nd, (int)ns, st, hist);
      hipLaunchKernelGGL(k_sel_final, dim3(1), dim3(256), 0, s, st, hist);
    }
    if (P->metric == GHICP_ICP_POINT_TO_POINT) {
      hipLaunchKernelGGL(k_acc_means, dim3(NBLK), dim3(256), 0, s, V, st, part);
      hipLaunchKernelGGL(k_icp_means, dim3(1), dim3(64), 0, s, st, part);
      hipLaunchKernelGGL(k_acc_cov, dim3(NBLK), dim3(256), 0, s, V, st, part);
    } else {
      hipLaunchKernelGGL(k_acc_plane, dim3(NBLK), dim3(256), 0, s, V, tnrm, st, part);
    }
    hipLaunchKernelGGL(k_icp_step, dim3(1), dim3(64), 0, s, st, part);
    hipLaunchKernelGGL(k_apply, dim3(gS), dim3(256), 0, s, cur, (int)ns, st);
    GH_HIP(hipMemcpyAsync(pin, st, sizeof(IcpState), hipMemcpyDeviceToHost, s));
    GH_HIP(hipStreamSynchronize(s));
    if (pin->converged || pin->reason == GHICP_ICP_NO_CORRESPONDENCES) break;
  }
  hst = *pin;
  stats->iterations = hst.iterations;
  stats->converged = hst.converged;
  stats->reason = hst.reason;
  stats->correspondences = hst.nv;
  stats->mse = hst.mse;
  memcpy(T16, hst.fin, sizeof(hst.fin));
  // output = final_transformation_ * input, then getFitnessScore() on it
  M16 M;
  memcpy(M.m, hst.fin, sizeof(M.m));
  hipLaunchKernelGGL(k_transform_f32, dim3(gS), dim3(256), 0, s, dS, (long long)ns, strideS, M, dOut, cur);
  GH_TRY(nn_search(ctx, XT, cur, (int)ns, nn, nd));
  hipLaunchKernelGGL(k_sum_f32, dim3(NBLK), dim3(256), 0, s, nd, (int)ns, part);
  double hp[NBLK];
  GH_HIP(hipMemcpyAsync(hp, part, sizeof(hp), hipMemcpyDeviceToHost, s));
  GH_HIP(hipStreamSynchronize(s));
  double f = 0;
  for (int b = 0; b < NBLK; b++) f += hp[b];
  stats->fitness = f / (double)ns;
  return sg.finish();
}

extern "C" int ghicp_gicp_params_default(ghicp_gicp_params* p) {
  if (!p) return GHICP_ERR_ARG;
  memset(p, 0, sizeof(*p));
  p->max_iter = 50;
  p->covariance_k = 20;
  p->thre_dis = 0.5f;
  p->min_overlap = 0.1f;
  p->max_inner_iter = 20;
  p->max_correspondence_distance = 1e6;  // common_reg.cpp:253
  p->gicp_epsilon = 1e-3;
  p->transformation_epsilon = 1e-8;      // common_reg.cpp:263
  p->rotation_epsilon = 1e-6;            // common_reg.cpp:265
  return GHICP_OK;
}

extern "C" int ghicp_gicp_covariances(ghicp_ctx* ctx, const float* xyz, int64_t n, int stride, int k, double eps, double* cov6) {
  GH_ENTER(ctx);
  GH_ARG(n >= 0 && n < (1ll << 31) - 2 && stride >= 3 && cov6 != nullptr && eps > 0.0);
  Stager sg(ctx);
  const float* d;
  double* o;
  GH_TRY(sg.in_cloud(xyz, (size_t)n * stride, &d));
  GH_TRY(sg.out(cov6, (size_t)n * 6, &o));
  GH_TRY(gh_gicp_cov_dev(ctx, d, n, stride, k, eps, o));
  return sg.finish();
}

extern "C" int ghicp_gicp(ghicp_ctx* ctx, const float* xyzS, int64_t ns, int strideS, const float* xyzT, int64_t nt, int strideT,
                          const ghicp_gicp_params* P, float* T16, float* transformed, ghicp_icp_stats* stats) {
  return ghicp_gicp_from(ctx, xyzS, ns, strideS, xyzT, nt, strideT, P, nullptr, T16, transformed, stats);
}

#define GICP_ARG(cond)                                                                 \
  do {                                                                                 \
    if (!(cond)) return ctx->fail(GHICP_ERR_ARG, "%s: bad argument (%s)", who, #cond); \
  } while (0)

// The body of ghicp_gicp_from and ghicp_gicp_trimmed_from (`who` names the one that was called).
// gicp_reg with transformation_ starting at guess16 (NULL: the identity, which is ghicp_gicp).  The source points and their covariances stay
// in the source's own frame: k_gicp_apply moves the points by transformation_, k_gicp_mahal rotates C_S by its R, k_gicp_prep takes x from it.
// trim: every outer iteration keeps the floor(ratio * count) correspondences with the smallest (d^2, index) of the count within the distance
// (trim_ratio in (0, 1], or 0 for the overlap the gate estimated); without it trim_ratio is not read and use_trimmed is the gate alone.
static int gicp_from_impl(ghicp_ctx* ctx, const char* who, const float* xyzS, int64_t ns, int strideS, const float* xyzT, int64_t nt, int strideT,
                          const ghicp_gicp_params* P, const float* guess16, bool trim, float trim_ratio, float* T16, float* transformed,
                          ghicp_icp_stats* stats) {
  GICP_ARG(P != nullptr && T16 != nullptr && stats != nullptr && ns >= 0 && nt >= 0 && ns < (1ll << 31) - 2 && nt < (1ll << 31) - 2 && strideS >= 3 &&
           strideT >= 3);
  GICP_ARG(P->covariance_k >= 1 && P->covariance_k <= 20 && P->max_inner_iter >= 1 && P->max_inner_iter <= 100);
  GICP_ARG(P->max_correspondence_distance > 0.0 && P->gicp_epsilon > 0.0 && P->transformation_epsilon > 0.0 && P->rotation_epsilon > 0.0);
  if (P->use_trimmed) GICP_ARG(P->thre_dis > 0.f);
  if (trim) {
    GICP_ARG(std::isfinite(trim_ratio) && trim_ratio >= 0.f && trim_ratio <= 1.f);
    if (trim_ratio == 0.f && !P->use_trimmed)
      return ctx->fail(GHICP_ERR_ARG, "%s: trim_ratio = 0 asks for the overlap estimate of the gate, which needs use_trimmed = 1", who);
  }
  const float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  float T0[16];
  memcpy(T0, guess16 ? guess16 : I16, sizeof(T0));
  for (int e = 0; e < 16; e++) GICP_ARG(std::isfinite(T0[e]));
  GICP_ARG(T0[12] == 0.f && T0[13] == 0.f && T0[14] == 0.f && T0[15] == 1.f);
  hipStream_t s = ctx->stream;
  memset(stats, 0, sizeof(*stats));
  Stager sg(ctx);
  const float *dS, *dT;
  float* dOut;
  GH_TRY(sg.in_cloud(xyzS, (size_t)ns * strideS, &dS));
  GH_TRY(sg.in_cloud(xyzT, (size_t)nt * strideT, &dT));
  GH_TRY(sg.out(transformed, (size_t)ns * 3, &dOut));

  float ratio = trim_ratio;
  if (P->use_trimmed) {  // common_reg.cpp:240-246: the only effect of the trimmed flag on gicp_reg (the rejector is never consulted)
    if (guess16 && ns > 0) {  // the gate sees the source where the guess puts it (the float expression of k_gicp_apply)
      float4* moved;
      GH_TRY(ctx->reserve(B_ICP_CUR, (size_t)ns + 1, &moved));
      M16 M;
      memcpy(M.m, T0, sizeof(M.m));
      hipLaunchKernelGGL(k_transform_f32, dim3(cdiv(ns, 256)), dim3(256), 0, s, dS, (long long)ns, strideS, M, (float*)nullptr, moved);
      GH_TRY(overlap_dev(ctx, reinterpret_cast<const float*>(moved), ns, 4, dT, nt, strideT, P->thre_dis, &ratio));
    } else {
      GH_TRY(overlap_dev(ctx, dS, ns, strideS, dT, nt, strideT, P->thre_dis, &ratio));
    }
    stats->overlap = ratio;
    if (ratio < P->min_overlap) { sg.outs.clear(); return GHICP_OK; }  // "This registration would not be done"
    if (trim_ratio != 0.f) ratio = trim_ratio;  // (0: the estimate feeds the rejector, as in icp_reg)
  }
  stats->done = 1;
  if (ns == 0 || nt == 0) {
    stats->reason = GHICP_ICP_NO_CORRESPONDENCES;
    memcpy(T16, T0, sizeof(T0));
    if (ns > 0 && dOut) {
      M16 M;
      memcpy(M.m, T0, sizeof(T0));
      hipLaunchKernelGGL(k_transform_f32, dim3(cdiv(ns, 256)), dim3(256), 0, s, dS, (long long)ns, strideS, M, dOut, (float4*)nullptr);
    }
    return sg.finish();
  }

  // everything the loop touches is reserved here: nothing allocates inside it
  float4 *src4, *cur, *tgt4;
  int* nn;
  float* nd;
  double *covS, *covT, *mahal, *part;
  GicpState* st;
  GicpSel* sel = nullptr;
  unsigned *pend, *hist = nullptr;
  GH_TRY(ctx->reserve(B_GICP_COVS, (size_t)ns * 6 + 6, &covS));
  GH_TRY(ctx->reserve(B_GICP_COVT, (size_t)nt * 6 + 6, &covT));
  GH_TRY(gh_gicp_cov_dev(ctx, dS, ns, strideS, P->covariance_k, P->gicp_epsilon, covS));
  GH_TRY(gh_gicp_cov_dev(ctx, dT, nt, strideT, P->covariance_k, P->gicp_epsilon, covT));
  GH_TRY(ctx->reserve(B_GICP_SRC4, (size_t)ns + 1, &src4));
  GH_TRY(ctx->reserve(B_GICP_MAHAL, (size_t)ns * 6 + 6, &mahal));
  GH_TRY(ctx->reserve(B_ICP_CUR, (size_t)ns + 1, &cur));
  GH_TRY(ctx->reserve(B_ICP_OUT, (size_t)nt + 1, &tgt4));
  GH_TRY(ctx->reserve(B_ICP_NN, (size_t)ns + 1, &nn));
  GH_TRY(ctx->reserve(B_ICP_ND, (size_t)ns + 1, &nd));
  GH_TRY(ctx->reserve(B_ICP_PART, (size_t)NBLK * NPART, &part));
  GH_TRY(ctx->reserve(B_ICP_STATE, 1, &st));
  if (trim) {
    GH_TRY(ctx->reserve(B_ICP_KEYS, (size_t)6 * SEL_BINS, &hist));
    GH_TRY(ctx->reserve(B_GICP_SEL, 1, &sel));
    GH_HIP(hipMemsetAsync(sel, 0, sizeof(GicpSel), s));
  }
  hipLaunchKernelGGL(k_pack4, dim3(cdiv(ns, 256)), dim3(256), 0, s, dS, (long long)ns, strideS, src4);
  hipLaunchKernelGGL(k_pack4, dim3(cdiv(nt, 256)), dim3(256), 0, s, dT, (long long)nt, strideT, tgt4);
  NnIndex XT;
  GH_TRY(build_index(ctx, dT, nt, strideT, 0.f, kSlotsTF, kSlotsTC, &XT, nullptr));
  GH_TRY(ctx->reserve(B_ICP_PEND, (size_t)ns + 4, &pend));  // nn_search's work list, at its final size before the loop

  GicpState hst;
  memset(&hst, 0, sizeof(hst));
  memcpy(hst.T, T0, sizeof(T0));
  hst.maxd2 = P->max_correspondence_distance * P->max_correspondence_distance;
  hst.inv_eps_r = 1.0 / P->rotation_epsilon;
  hst.inv_eps_t = 1.0 / P->transformation_epsilon;
  hst.max_iter = P->max_iter;
  hst.ratio = trim ? ratio : 0.f;
  GH_HIP(hipMemcpyAsync(st, &hst, sizeof(hst), hipMemcpyHostToDevice, s));
  GicpState* pin = reinterpret_cast<GicpState*>(ctx->pinned);
  static_assert(sizeof(GicpState) <= 4096, "status record must fit the pinned scratch");
  const int gS = cdiv(ns, 256);
  const int gSel = min(cdiv(ns, 2048), 512);
  for (;;) {
    hipLaunchKernelGGL(k_gicp_apply, dim3(gS), dim3(256), 0, s, src4, (int)ns, st, cur);
    GH_TRY(nn_search(ctx, XT, cur, (int)ns, nn, nd));
    if (trim) {
      hipLaunchKernelGGL(k_gicp_reject, dim3(gS), dim3(256), 0, s, nn, nd, (int)ns, st, sel);
      hipLaunchKernelGGL(k_gicp_trim_prep, dim3(1), dim3(1), 0, s, st, sel);
      hipEvent_t kt = ctx->kt_begin(KT_GICP_SELECT);
      GH_HIP(hipMemsetAsync(hist, 0, (size_t)6 * SEL_BINS * sizeof(unsigned), s));
      for (int pass = 0; pass < 6; pass++) hipLaunchKernelGGL(k_gicp_sel_pass, dim3(gSel), dim3(256), 0, s, pass, nn, nd, (int)ns, sel, hist);
      hipLaunchKernelGGL(k_gicp_sel_final, dim3(1), dim3(256), 0, s, sel, hist);
      ctx->kt_end(KT_GICP_SELECT, kt);
      hipLaunchKernelGGL(k_gicp_mahal_trim, dim3(NBLK), dim3(256), 0, s, nn, nd, (int)ns, covS, covT, st, sel, mahal, part);
    } else {
      hipLaunchKernelGGL(k_gicp_mahal, dim3(NBLK), dim3(256), 0, s, nn, nd, (int)ns, covS, covT, st, mahal, part);
    }
    hipLaunchKernelGGL(k_gicp_prep, dim3(1), dim3(64), 0, s, st, part);
    for (int k = 0; k < P->max_inner_iter; k++) {
      hipLaunchKernelGGL(k_gicp_acc, dim3(NBLK), dim3(256), 0, s, src4, tgt4, nn, (int)ns, mahal, st, part);
      hipLaunchKernelGGL(k_gicp_solve, dim3(1), dim3(64), 0, s, st, part);
    }
    hipLaunchKernelGGL(k_gicp_outer, dim3(1), dim3(1), 0, s, st);
    GH_HIP(hipGetLastError());
    GH_HIP(hipMemcpyAsync(pin, st, sizeof(GicpState), hipMemcpyDeviceToHost, s));
    GH_HIP(hipStreamSynchronize(s));
    if (pin->converged || pin->reason == GHICP_ICP_NO_CORRESPONDENCES) break;
  }
  hst = *pin;
  stats->iterations = hst.iterations;
  stats->converged = hst.converged;
  stats->reason = hst.reason;
  stats->correspondences = hst.count;
  stats->mse = hst.mse;
  memcpy(T16, hst.T, sizeof(hst.T));
  // output = final_transformation_ * input, then getFitnessScore() on it
  M16 M;
  memcpy(M.m, hst.T, sizeof(M.m));
  hipLaunchKernelGGL(k_transform_f32, dim3(gS), dim3(256), 0, s, dS, (long long)ns, strideS, M, dOut, cur);
  GH_TRY(nn_search(ctx, XT, cur, (int)ns, nn, nd));
  hipLaunchKernelGGL(k_sum_f32, dim3(NBLK), dim3(256), 0, s, nd, (int)ns, part);
  double hp[NBLK];
  GH_HIP(hipMemcpyAsync(hp, part, sizeof(hp), hipMemcpyDeviceToHost, s));
  GH_HIP(hipStreamSynchronize(s));
  double f = 0;
  for (int b = 0; b < NBLK; b++) f += hp[b];
  stats->fitness = f / (double)ns;
  return sg.finish();
}

extern "C" int ghicp_gicp_from(ghicp_ctx* ctx, const float* xyzS, int64_t ns, int strideS, const float* xyzT, int64_t nt, int strideT,
                               const ghicp_gicp_params* P, const float* guess16, float* T16, float* transformed, ghicp_icp_stats* stats) {
  GH_ENTER(ctx);
  return gicp_from_impl(ctx, "ghicp_gicp_from", xyzS, ns, strideS, xyzT, nt, strideT, P, guess16, false, 1.0f, T16, transformed, stats);
}

extern "C" int ghicp_gicp_trimmed_from(ghicp_ctx* ctx, const float* xyzS, int64_t ns, int strideS, const float* xyzT, int64_t nt, int strideT,
                                       const ghicp_gicp_params* P, const float* guess16, float trim_ratio, float* T16, float* transformed,
                                       ghicp_icp_stats* stats) {
  GH_ENTER(ctx);
  return gicp_from_impl(ctx, "ghicp_gicp_trimmed_from", xyzS, ns, strideS, xyzT, nt, strideT, P, guess16, true, trim_ratio, T16, transformed, stats);
}
