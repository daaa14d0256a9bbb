// CFilter's cleaning filters on gfx950 (reference include/filter.hpp:90-140): SORFilter = pcl::StatisticalOutlierRemoval, DisFilter,
// ActiveObjectFilter.  The contract is in include/ghicp_c.h and DESIGN.md N9 / Q10 / Q11:
//   k_sor_knn       one wavefront per query point (queries in cell order): ring expansion over the uniform grid with knn_point's stopping
//                   rule, 64 candidates per step (one per lane), the 64 smallest d2 seen so far held sorted, one per lane; a step in which
//                   no candidate beats the current (mean_k + 1)-th is skipped after one ballot, otherwise the candidates are sorted by a
//                   bitonic network and merged in.  Only distances are kept.  Epilogue: sqrtf per lane, f64 sum in ascending order.
//   k_sor_partials  (sum, sum of squares) of every tile of SOR_TILE consecutive distances, in index order (N9); the tiles are added in index
//                   order on the host, which also takes the square root -- the threshold is the restatement's bit for bit
//   flag kernels    one byte per point, compacted by the library's own select (prims.hip)
#include "frontend.h"
#include "prims.h"

namespace {

constexpr int SOR_TILE = 1024;    // N9: distances per partial sum
constexpr int SOR_MAX_K = 63;     // the query and its neighbours fill at most the 64 lanes of a wave
constexpr int SOR_WAVES = 4;      // queries per workgroup

// ascending bitonic sort of one value per lane over the 64 lanes of a wave (21 compare-exchange steps)
__device__ inline float wave_sort64(float v, int lane) {
  for (int k = 2; k <= 64; k <<= 1)
    for (int j = k >> 1; j >= 1; j >>= 1) {
      const float o = __shfl_xor(v, j);
      const bool take_min = ((lane & j) == 0) == ((lane & k) == 0);
      v = (take_min == (o < v)) ? o : v;
    }
  return v;
}

__global__ __launch_bounds__(64 * SOR_WAVES) void k_sor_knn(GridArgs G, float cell, int K, float* __restrict__ dist) {
  const int lane = threadIdx.x & 63;
  const long long p = blockIdx.x * (long long)SOR_WAVES + (threadIdx.x >> 6);
  if (p >= G.d.n) return;  // a whole wave
  const float4 P = G.pts[p];
  const int self = (int)__float_as_uint(P.w);
  // the same for every lane: say so, and the walk over the cells below is scalar
  const int cx = __builtin_amdgcn_readfirstlane(gh_cell_coord(P.x, G.d.mn[0], G.d.inv, G.d.dim[0]));
  const int cy = __builtin_amdgcn_readfirstlane(gh_cell_coord(P.y, G.d.mn[1], G.d.inv, G.d.dim[1]));
  const int cz = __builtin_amdgcn_readfirstlane(gh_cell_coord(P.z, G.d.mn[2], G.d.inv, G.d.dim[2]));
  float best = INFINITY;   // lane t: the t-th smallest d2 so far
  float worst = INFINITY;  // lane K - 1's entry
  auto scan_run = [&](unsigned b, unsigned e) {  // the points [b, e) of the cell-ordered array
    for (unsigned q0 = b; q0 < e; q0 += 64u) {
      const unsigned q = q0 + (unsigned)lane;
      float d2 = INFINITY;
      if (q < e) {
        const float4 Q = G.pts[q];
        const float dx = P.x - Q.x, dy = P.y - Q.y, dz = P.z - Q.z;
        d2 = dx * dx;
        d2 += dy * dy;
        d2 += dz * dz;
      }
      if (__ballot(d2 < worst) == 0ull) continue;
      // best ascending, candidates descending: the lane-wise minimum holds the 64 smallest of the 128 as a bitonic sequence
      const float c = __shfl(wave_sort64(d2, lane), 63 - lane);
      best = c < best ? c : best;
      for (int j = 32; j >= 1; j >>= 1) {
        const float o = __shfl_xor(best, j);
        best = (((lane & j) == 0) == (o < best)) ? o : best;
      }
      worst = __shfl(best, K - 1);
    }
  };
  const int rmax = max(G.d.dim[0], max(G.d.dim[1], G.d.dim[2]));
  for (int r = 0; r <= rmax; r++) {
    const int x0 = max(cx - r, 0), x1 = min(cx + r, G.d.dim[0] - 1);
    const int y0 = max(cy - r, 0), y1 = min(cy + r, G.d.dim[1] - 1);
    const int z0 = max(cz - r, 0), z1 = min(cz + r, G.d.dim[2] - 1);
    for (int x = x0; x <= x1; x++)
      for (int y = y0; y <= y1; y++) {
        const unsigned base = ((unsigned)x * G.d.dim[1] + y) * G.d.dim[2];
        if ((abs(x - cx) == r) || (abs(y - cy) == r)) {  // rim column of shell r: its cells z0 .. z1 are one run of the point array
          scan_run(G.start[base + z0], G.start[base + z1 + 1]);
        } else {  // interior column: only the two caps
          if (cz - r >= 0) scan_run(G.start[base + cz - r], G.start[base + cz - r + 1]);
          if (cz + r <= G.d.dim[2] - 1) scan_run(G.start[base + cz + r], G.start[base + cz + r + 1]);
        }
      }
    if (r >= 1) {
      // every unscanned point is at least r cells away (knn_point's rule); a thousandth of a cell covers the float rounding of the cell coordinates
      const float reach = ((float)r - 1e-3f) * cell;
      if (worst < reach * reach) break;
    }
  }
  // entry 0 is the query itself (or a duplicate of it); entries 1 .. K - 1 in ascending order, f64
  const int sq = __float_as_int(sqrtf(best));
  double sum = 0.0;
  for (int t = 1; t < K; t++) sum += (double)__int_as_float(__builtin_amdgcn_readlane(sq, t));
  if (lane == 0) dist[self] = (float)(sum / (double)(K - 1));
}

__global__ __launch_bounds__(64) void k_sor_partials(const float* __restrict__ dist, long long n, double* __restrict__ part) {
  const long long t = blockIdx.x * 64ll + threadIdx.x;
  const long long b = t * SOR_TILE;
  if (b >= n) return;
  const long long e = b + SOR_TILE < n ? b + SOR_TILE : n;
  double s = 0.0, q = 0.0;
  for (long long i = b; i < e; i++) {
    const double d = (double)dist[i];
    s += d;
    q += d * d;
  }
  part[2 * t] = s;
  part[2 * t + 1] = q;
}

__global__ __launch_bounds__(256) void k_sor_flags(const float* __restrict__ dist, long long n, double threshold, unsigned char* __restrict__ flags) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  flags[i] = !((double)dist[i] > threshold) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_iota(int* __restrict__ out, long long n) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i < n) out[i] = (int)i;
}

// filter.hpp:110-111 as written (Q10): x * x + y + y in float, compared in double
__global__ __launch_bounds__(256) void k_dis_flags(const float* __restrict__ xyz, long long n, int stride, double xy_max2, double z_min, double z_max,
                                                   unsigned char* __restrict__ flags) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const float x = xyz[i * stride], y = xyz[i * stride + 1], z = xyz[i * stride + 2];
  float e = x * x;
  e += y;
  e += y;
  const double dis_square = (double)e;
  flags[i] = (dis_square < xy_max2 && (double)z < z_max && (double)z > z_min) ? 1 : 0;
}

// filter.hpp:121-137 (Q11): a point strictly inside any box leaves
__global__ __launch_bounds__(256) void k_box_flags(const float* __restrict__ xyz, long long n, int stride, const double* __restrict__ boxes, int n_boxes,
                                                   unsigned char* __restrict__ flags) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const double x = (double)xyz[i * stride], y = (double)xyz[i * stride + 1], z = (double)xyz[i * stride + 2];
  unsigned char keep = 1;
  for (int j = 0; j < n_boxes; j++) {
    const double* b = boxes + (size_t)j * 6;
    if (x > b[0] && x < b[3] && y > b[1] && y < b[4] && z > b[2] && z < b[5]) { keep = 0; break; }
  }
  flags[i] = keep;
}

// dist[i] of every point, n >= mean_k + 1
int sor_knn_dev(ghicp_ctx* ctx, const float* xyz, long long n, int stride, int mean_k, float* dist) {
  float mm[6];
  GH_TRY(gh_bbox_dev(ctx, xyz, n, stride, mm));
  const float cell = gh_fpfh_cell(mm, n);
  DeviceGrid G;
  const GridSlots sl = {B_GRID2_KEYS, B_GRID2_KEYS2, B_GRID2_VALS, B_GRID2_VALS2, B_GRID2_START, B_GRID2_PTS};
  GH_TRY(gh_grid_build(ctx, xyz, n, stride, cell, sl, &G));
  GridArgs A = {G.d, G.pts, G.start};
  hipLaunchKernelGGL(k_sor_knn, dim3(cdiv(n, SOR_WAVES)), dim3(64 * SOR_WAVES), 0, ctx->stream, A, 1.0f / G.d.inv, mean_k + 1, dist);
  GH_HIP(hipGetLastError());
  return GHICP_OK;
}

// keep = the positions of the set flags, *m_out = their number (synchronises)
int select_kept(ghicp_ctx* ctx, const unsigned char* flags, long long n, int32_t* keep, long long* m_out) {
  int* dcount;
  GH_TRY(ctx->reserve(B_FE_SCAN, 16, &dcount));
  GH_TRY(gh_select_flagged_iota(ctx, flags, n, keep, dcount));
  int* hc = reinterpret_cast<int*>(reinterpret_cast<char*>(ctx->pinned) + 320);  // pinned: see gh_bbox_dev
  GH_HIP(hipMemcpyAsync(hc, dcount, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  GH_HIP(hipStreamSynchronize(ctx->stream));
  *m_out = (long long)*hc;
  return GHICP_OK;
}

int sor_filter_dev(ghicp_ctx* ctx, const float* xyz, long long n, int stride, int mean_k, double std_mul, int32_t* keep, long long* m_out, double* stats4) {
  hipStream_t s = ctx->stream;
  const double nan = std::nan("");
  stats4[0] = stats4[1] = stats4[2] = nan;
  stats4[3] = 0.0;
  *m_out = 0;
  if (n <= 0) return GHICP_OK;
  if (n < (long long)mean_k + 1) {  // PCL: short result lists, no valid distance, NaN threshold -- every point stays
    hipLaunchKernelGGL(k_iota, dim3(cdiv(n, 256)), dim3(256), 0, s, keep, n);
    GH_HIP(hipGetLastError());
    GH_HIP(hipStreamSynchronize(s));
    *m_out = n;
    return GHICP_OK;
  }
  float* dist;
  double* part;
  unsigned char* flags;
  const long long nt = (n + SOR_TILE - 1) / SOR_TILE;
  GH_TRY(ctx->reserve(B_SOR_DIST, (size_t)n + 4, &dist));
  GH_TRY(ctx->reserve(B_SOR_PART, (size_t)nt * 2 + 2, &part));
  GH_TRY(ctx->reserve(B_FE_FLAGS, (size_t)n + 16, &flags));
  GH_TRY(sor_knn_dev(ctx, xyz, n, stride, mean_k, dist));
  hipLaunchKernelGGL(k_sor_partials, dim3(cdiv(nt, 64)), dim3(64), 0, s, dist, n, part);
  GH_HIP(hipGetLastError());
  std::vector<double> hp((size_t)nt * 2);
  GH_HIP(hipMemcpyAsync(hp.data(), part, hp.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  GH_HIP(hipStreamSynchronize(s));
  double sum = 0.0, sq_sum = 0.0;  // N9: the tiles in index order
  for (long long t = 0; t < nt; t++) {
    sum += hp[(size_t)t * 2];
    sq_sum += hp[(size_t)t * 2 + 1];
  }
  const double dn = (double)n;
  const double mean = sum / dn;
  const double variance = (sq_sum - sum * sum / dn) / (dn - 1.0);
  const double stddev = std::sqrt(variance);
  const double threshold = mean + std_mul * stddev;
  stats4[0] = mean; stats4[1] = stddev; stats4[2] = threshold; stats4[3] = dn;
  hipLaunchKernelGGL(k_sor_flags, dim3(cdiv(n, 256)), dim3(256), 0, s, dist, n, threshold, flags);
  GH_HIP(hipGetLastError());
  return select_kept(ctx, flags, n, keep, m_out);
}

}  // namespace

#define GH_CLOUD_ARGS(n, stride)                                                                                                   \
  do {                                                                                                                             \
    if ((n) >= (1ll << 31) - 2) return ctx->fail(GHICP_ERR_CAPACITY, "%s: n = %lld exceeds the 2^31 - 3 points of an int32 index", __func__, (long long)(n)); \
    GH_ARG((n) >= 0 && ((stride) == 3 || (stride) == 4 || (stride) == 8));                                                         \
  } while (0)

extern "C" int ghicp_knn_mean_distance(ghicp_ctx* ctx, const float* xyz, int64_t n, int stride, int mean_k, float* dist) {
  GH_ENTER(ctx);
  GH_CLOUD_ARGS(n, stride);
  if (mean_k < 1 || mean_k > SOR_MAX_K) return ctx->fail(GHICP_ERR_ARG, "ghicp_knn_mean_distance: mean_k must be in [1, %d]", SOR_MAX_K);
  GH_ARG(n == 0 || (xyz != nullptr && dist != nullptr));
  if (n == 0) return GHICP_OK;
  Stager sg(ctx);
  const float* d;
  float* dd;
  GH_TRY(sg.in_cloud(xyz, (size_t)n * stride, &d));
  GH_TRY(sg.out(dist, (size_t)n, &dd));
  if (n < (int64_t)mean_k + 1) GH_HIP(hipMemsetAsync(dd, 0, (size_t)n * sizeof(float), ctx->stream));  // PCL: distances[i] = 0 on a short result list
  else GH_TRY(sor_knn_dev(ctx, d, n, stride, mean_k, dd));
  return sg.finish();
}

extern "C" int ghicp_sor_filter(ghicp_ctx* ctx, const float* xyz, int64_t n, int stride, int mean_k, double std_mul, int32_t* keep_idx, int64_t* m,
                                double* stats4) {
  GH_ENTER(ctx);
  GH_CLOUD_ARGS(n, stride);
  if (mean_k < 1 || mean_k > SOR_MAX_K) return ctx->fail(GHICP_ERR_ARG, "ghicp_sor_filter: mean_k must be in [1, %d]", SOR_MAX_K);
  GH_ARG(m != nullptr && (n == 0 || (xyz != nullptr && keep_idx != nullptr)));
  Stager sg(ctx);
  const float* d;
  int32_t* k;
  GH_TRY(sg.in_cloud(xyz, (size_t)n * stride, &d));
  GH_TRY(sg.out(keep_idx, (size_t)n, &k));
  long long mm = 0;
  double st[4];
  GH_TRY(sor_filter_dev(ctx, d, n, stride, mean_k, std_mul, k, &mm, st));
  *m = mm;
  if (stats4) memcpy(stats4, st, sizeof(st));
  return sg.finish();
}

extern "C" int ghicp_dis_filter(ghicp_ctx* ctx, const float* xyz, int64_t n, int stride, double xy_dis_max, double z_min, double z_max, int32_t* keep_idx,
                                int64_t* m) {
  GH_ENTER(ctx);
  GH_CLOUD_ARGS(n, stride);
  GH_ARG(m != nullptr && (n == 0 || (xyz != nullptr && keep_idx != nullptr)));
  *m = 0;
  if (n == 0) return GHICP_OK;
  Stager sg(ctx);
  const float* d;
  int32_t* k;
  unsigned char* flags;
  GH_TRY(sg.in_cloud(xyz, (size_t)n * stride, &d));
  GH_TRY(sg.out(keep_idx, (size_t)n, &k));
  GH_TRY(ctx->reserve(B_FE_FLAGS, (size_t)n + 16, &flags));
  hipLaunchKernelGGL(k_dis_flags, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, d, n, stride, xy_dis_max * xy_dis_max, z_min, z_max, flags);
  GH_HIP(hipGetLastError());
  long long mm = 0;
  GH_TRY(select_kept(ctx, flags, n, k, &mm));
  *m = mm;
  return sg.finish();
}

extern "C" int ghicp_box_filter(ghicp_ctx* ctx, const float* xyz, int64_t n, int stride, const double* boxes6, int32_t n_boxes, int32_t* keep_idx,
                                int64_t* m) {
  GH_ENTER(ctx);
  GH_CLOUD_ARGS(n, stride);
  GH_ARG(m != nullptr && n_boxes >= 0 && (n_boxes == 0 || boxes6 != nullptr) && (n == 0 || (xyz != nullptr && keep_idx != nullptr)));
  *m = 0;
  if (n == 0) return GHICP_OK;
  Stager sg(ctx);
  const float* d;
  int32_t* k;
  unsigned char* flags;
  double* boxes;
  GH_TRY(sg.in_cloud(xyz, (size_t)n * stride, &d));
  GH_TRY(sg.out(keep_idx, (size_t)n, &k));
  GH_TRY(ctx->reserve(B_FE_FLAGS, (size_t)n + 16, &flags));
  GH_TRY(ctx->reserve(B_SOR_PART, (size_t)n_boxes * 6 + 2, &boxes));
  if (n_boxes > 0) GH_TRY(ctx->upload_table(boxes6, (size_t)n_boxes * 6 * sizeof(double), boxes));
  hipLaunchKernelGGL(k_box_flags, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, d, n, stride, boxes, (int)n_boxes, flags);
  GH_HIP(hipGetLastError());
  long long mm = 0;
  GH_TRY(select_kept(ctx, flags, n, k, &mm));
  *m = mm;
  return sg.finish();
}
