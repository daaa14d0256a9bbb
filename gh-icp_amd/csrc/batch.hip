// Batched per-cloud front end (gfx950): nb clouds go through down-sampling, keypoint detection and BSC encoding
// (test/ghicp_main.cpp:86-127 per cloud; FPFH rows instead of BSC strings for Ft = F) with ONE sequence of launches.
//
// Why: one cloud's front end is ~100 device operations (24 kernels, 3 radix sorts, 4 selects, copies, 7 host synchronisations that size
// the next stage) and the host issues them at ~8 us each, so a cloud costs 0.85 ms however many streams submit clouds.
// Here the clouds of a batch are CONCATENATED: every elementwise kernel, sort and select runs once over all their points, and the kernels
// that work per cell / per keypoint (gh_pca_cell_body, gh_bsc_keypoint -- the same device code as the single-cloud path) look their cloud
// up in a descriptor block.
//   * voxel keys carry the cloud id above the voxel key's bits; the clouds are the segments of ONE stable radix sort (prims.hip: every cloud
//     sorted among its own points inside the same launches, on the voxel key's bits alone), so clouds stay apart and ordered;
//   * grid cells are numbered globally (cell base of the cloud + cell) -> one segmented sort (on the cell inside the cloud's grid) / one cell
//     table per grid for all clouds;
//   * NMS: decision rounds with one thread per candidate over every cloud of the batch, not the one-workgroup sweep of the single-cloud
//     path (batch_nms.hip has the design).
// FPFH clouds: the kNN grid is the batch's second grid and the normal / SPFH / FPFH kernels of fpfh.hip run once over the concatenated cloud.
// Host synchronisations of a batch: three reports that size the next stage (raw boxes; down-sampled counts and boxes; candidate counts),
// one per launch sequence of FB_NMS_ROUNDS NMS rounds (one sequence settles a scan), and the last one before the handles are handed back.
// Results are bit-identical to ghicp_cloud_recompute() cloud by cloud: same per-cloud boxes, same grids, same orders inside a cell,
// same reduction trees (tests/test_gpu_batch.py).
// Where things live: batch_dev.h has the descriptor block, the report and the state of a batch in flight (FbRun); batch_nms.hip the NMS
// rounds; this file the other kernels, one host function per stage (fb_*, in the order they run) and the C entry point.
#include "batch_dev.h"
#include "frontend.h"
#include "pca_dev.h"
#include "bsc_dev.h"
#include "prims.h"

#include <cmath>

namespace {

enum { FB_CLOUD_BY_CLOUD = -1, FB_HALVE = -2 };  // a stage's verdict that the batch as it stands is not covered: the entry point takes the fall-back

// per-cloud bounding boxes; which = 0: raw clouds, 1: base = concatenated float4 points (moff), 2: base = float3 candidates (coff)
__global__ __launch_bounds__(256) void k_fb_bbox(const FbBlock* __restrict__ D, const float* __restrict__ base, int which, int* __restrict__ bb) {
  const int b = blockIdx.y;
  const float* xyz;
  long long n;
  int stride;
  if (which == 0) { xyz = D->c[b].xyz; n = D->c[b].n; stride = D->c[b].stride; }
  else {
    const int* off = which == 1 ? D->moff : D->coff;
    stride = which == 1 ? 4 : 3;
    xyz = base + (size_t)off[b] * stride;
    n = off[b + 1] - off[b];
  }
  if (n <= 0) return;
  float mn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, mx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    for (int d = 0; d < 3; d++) { const float v = xyz[i * stride + d]; mn[d] = fminf(mn[d], v); mx[d] = fmaxf(mx[d], v); }
  gh_box_block(mn, mx, bb + b * 6);
}

// filter.hpp:57-70 per cloud; the cloud id sits above the voxel key's bits
// idx_bits > 0 (branch next/fe-packed-voxel-sort): the point's index rides in the low bits of the key itself -- ONE 8-byte array goes through the
// radix sort (keys only, sorted on the bits above the index: stable, so the lowest index still leads its voxel) instead of a key and a value array
// One workgroup per tile of the voxel sort's partition (sort_plan.h: tiles never cross a cloud, so the tile's segment IS the cloud); F.table != nullptr:
// the tile's counts of the sort's first digit place are taken on the way (gh_rs_first_*, prims.h) and the sort skips its first histogram pass
__global__ __launch_bounds__(256) void k_fb_voxel_keys(const FbBlock* __restrict__ D, GhRsSegs S, int shift, int idx_bits, unsigned long long* __restrict__ keys,
                                                       unsigned* __restrict__ vals, GhRsFirst F) {
  __shared__ unsigned cnt[4][GH_RS_MAX_ND];
  const bool hist = F.table != nullptr;
  if (hist) gh_rs_first_zero(cnt, F.nd);
  const GhRsTile t = gh_rs_tile(S, (int)blockIdx.x);
  const int b = t.seg;
  const FbCloud& C = D->c[b];
  const float* base = C.xyz + (size_t)(t.first - S.off[b]) * C.stride;
#pragma unroll 4
  for (int k = 0; k < GH_RS_TILE / 256; k++) {
    const int j = k * 256 + (int)threadIdx.x;
    if (j < t.here) {
      const int i = t.first + j;
      const float* p = base + (size_t)j * C.stride;
      const unsigned long long vx = (unsigned long long)floorf((p[0] - C.vmn[0]) * C.vinv);
      const unsigned long long vy = (unsigned long long)floorf((p[1] - C.vmn[1]) * C.vinv);
      const unsigned long long vz = (unsigned long long)floorf((p[2] - C.vmn[2]) * C.vinv);
      const unsigned long long vox = vx * C.mul_x + vy * C.mul_y + vz;
      const unsigned long long key = ((unsigned long long)b << shift) | vox;
      if (idx_bits > 0) keys[i] = (key << idx_bits) | (unsigned long long)i;
      else { keys[i] = key; vals[i] = (unsigned)i; }
      if (hist) gh_rs_first_add(cnt, (unsigned)vox & F.mask);
    }
  }
  if (hist) gh_rs_first_store(cnt, F, (int)blockIdx.x);
}

// head of every voxel run whose voxel key > 0 (the run of voxel 0 is the reference's phantom group: filter.hpp:52,66,75-83)
__global__ __launch_bounds__(256) void k_fb_voxel_flags(const unsigned long long* __restrict__ keys, int N, unsigned long long vmask, int idx_bits,
                                                        unsigned char* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const unsigned long long k = keys[i] >> idx_bits;
  flags[i] = ((k & vmask) != 0ull && (i == 0 || (keys[i - 1] >> idx_bits) != k)) ? 1 : 0;
}

__device__ inline int fb_lower_bound(const int* __restrict__ a, int n, int v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// heads per cloud (sorted positions are grouped by cloud) and the offsets of the down-sampled clouds: heads + the phantom row
__global__ __launch_bounds__(128) void k_fb_voxel_bounds(const int* __restrict__ headpos, const int* __restrict__ total, FbBlock* D, FbOut* O) {
  const int nb = D->nb, t = threadIdx.x;
  if (t <= nb) { const int v = fb_lower_bound(headpos, *total, D->roff[t]); D->hoff[t] = v; O->hoff[t] = v; }
  __syncthreads();
  if (t == 0) {
    int acc = 0;
    for (int b = 0; b <= nb; b++) {
      D->moff[b] = acc; O->moff[b] = acc;
      if (b < nb) acc += (D->hoff[b + 1] - D->hoff[b]) + (D->c[b].n > 0 ? 1 : 0);
    }
  }
}

// candidates per cloud (ascending global point index)
__global__ __launch_bounds__(128) void k_fb_cand_bounds(const int* __restrict__ cand, const int* __restrict__ total, FbBlock* D, FbOut* O) {
  const int t = threadIdx.x;
  if (t <= D->nb) { const int v = fb_lower_bound(cand, *total, D->moff[t]); D->coff[t] = v; O->coff[t] = v; }
}

// down-sampled clouds, concatenated: row 0 of a cloud is its raw point 0 (phantom group), then the lowest-index point of every voxel
__global__ __launch_bounds__(256) void k_fb_gather_ds(const FbBlock* __restrict__ D, const int* __restrict__ headpos, const unsigned* __restrict__ vals2,
                                                      const unsigned long long* __restrict__ packed, unsigned long long idx_mask, float4* __restrict__ dsg) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int nb = D->nb;
  if (i >= D->moff[nb]) return;
  const int b = fb_find(D->moff, nb, i), j = i - D->moff[b];
  const FbCloud& C = D->c[b];
  long long s = 0;
  if (j != 0) {
    const int hp = headpos[D->hoff[b] + j - 1];
    s = (packed ? (long long)(packed[hp] & idx_mask) : (long long)vals2[hp]) - D->roff[b];
  }
  const float* p = C.xyz + (size_t)s * C.stride;
  dsg[i] = make_float4(p[0], p[1], p[2], 0.f);
}

// one workgroup per tile of the grid sort's partition (the tile's segment is the cloud); the first place's counts as in k_fb_voxel_keys
__global__ __launch_bounds__(256) void k_fb_cell_keys(const FbBlock* __restrict__ D, int which, const float4* __restrict__ dsg, GhRsSegs S,
                                                      unsigned* __restrict__ keys, unsigned* __restrict__ vals, GhRsFirst F) {
  __shared__ unsigned cnt[4][GH_RS_MAX_ND];
  const bool hist = F.table != nullptr;
  if (hist) gh_rs_first_zero(cnt, F.nd);
  const GhRsTile t = gh_rs_tile(S, (int)blockIdx.x);
  const int b = t.seg;
  const GridDesc& g = which ? D->g2[b] : D->g1[b];
  const unsigned cb = which ? D->cb2[b] : D->cb1[b];
#pragma unroll 4
  for (int k = 0; k < GH_RS_TILE / 256; k++) {
    const int j = k * 256 + (int)threadIdx.x;
    if (j < t.here) {
      const int i = t.first + j;
      const float4 P = dsg[i];
      const unsigned cell = gh_cell_key(g, P.x, P.y, P.z);
      keys[i] = cb + cell;
      vals[i] = (unsigned)i;
      if (hist) gh_rs_first_add(cnt, cell & F.mask);
    }
  }
  if (hist) gh_rs_first_store(cnt, F, (int)blockIdx.x);
}

// pca.hip:k_pca_cells over the occupied cells of all clouds of the batch
template <int CHUNK>
__global__ __launch_bounds__(64) void k_fb_pca_cells(const FbBlock* __restrict__ D, const float4* __restrict__ pts, const unsigned* __restrict__ start,
                                                      const unsigned* __restrict__ cells, const int* __restrict__ ncells, int* __restrict__ counter,
                                                      float r2, double* __restrict__ scat, int* __restrict__ count) {
  __shared__ float4 sC[CHUNK];
  const int lane = threadIdx.x;
  const int nc = *ncells;
  // cell bases of the clouds into LDS: the cloud of a cell is found there (rounds 3-4: a binary search through global memory per cell)
  __shared__ unsigned s_cb[FB_MAX + 1];
  const int nbc = D->nb;
  for (int i = lane; i <= nbc; i += 64) s_cb[i] = D->cb1[i];
  __syncthreads();
  auto cloud_of = [&](unsigned gkey) {
    int lo = 0, hi = nbc - 1;  // last b with s_cb[b] <= gkey
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (s_cb[mid] <= gkey) lo = mid;
      else hi = mid - 1;
    }
    return lo;
  };
  // static deal of the occupied cells: runs of 8 consecutive cells, neighbourhoods per XCD (pca_dev.h).  Within a run the cloud and its
  // grid are looked up once (they change at most once per cloud), and every cell's table lookups are issued one cell ahead.
  gh_pca_for_my_runs(nc, counter, [&](int c0, int cnt) {
    const unsigned key_l = lane < cnt ? cells[c0 + lane] : 0u;
    unsigned gkey = (unsigned)__builtin_amdgcn_readlane((int)key_l, 0);
    int b = cloud_of(gkey);
    GridArgs G;
    G.d = D->g1[b]; G.pts = pts; G.start = start + s_cb[b];
    unsigned cb_lo = s_cb[b], cb_hi = s_cb[b + 1];
    PcaMeta mn = gh_pca_meta(G, gkey - cb_lo, lane);
    for (int j = 0; j < cnt; j++) {
      const PcaMeta m = mn;
      const GridArgs Gc = G;
      const unsigned keyc = gkey - cb_lo;
      if (j + 1 < cnt) {
        gkey = (unsigned)__builtin_amdgcn_readlane((int)key_l, j + 1);
        if (gkey >= cb_hi) {  // the run crosses into the next cloud
          b = cloud_of(gkey);
          G.d = D->g1[b]; G.start = start + s_cb[b];
          cb_lo = s_cb[b]; cb_hi = s_cb[b + 1];
        }
        mn = gh_pca_meta(G, gkey - cb_lo, lane);
      }
      __syncthreads();
      gh_pca_cell_body<CHUNK>(Gc, keyc, m, r2, scat, count, sC, lane);
    }
  });
}

__global__ __launch_bounds__(256) void k_fb_pca_eigen(const double* __restrict__ scat, const int* __restrict__ count, int m, float* __restrict__ lambda,
                                                      double* __restrict__ curvature) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < m) gh_pca_eigen_point(scat, count, i, lambda, curvature);
}

// keypoint_detect.hpp:132-147 (pca.hip:k_prune_flags)
__global__ __launch_bounds__(256) void k_fb_prune_flags(const float* __restrict__ lambda, const int* __restrict__ count, int m, float ratio_max, int min_n,
                                                        unsigned char* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const double l1 = (double)lambda[(size_t)i * 3], l2 = (double)lambda[(size_t)i * 3 + 1], l3 = (double)lambda[(size_t)i * 3 + 2];
  const float r1 = (float)(l2 / l1), r2 = (float)(l3 / l2);
  flags[i] = (r1 < ratio_max && r2 < ratio_max && count[i] > min_n) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_fb_copy_ds(const FbBlock* __restrict__ D, const float4* __restrict__ dsg, int M) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const int b = fb_find(D->moff, D->nb, i);
  D->c[b].ds[i - D->moff[b]] = dsg[i];
}

// keypoint ids, coordinates as f64 (dataio.hpp:609-627) and the LCS origins of the BSC encoder (bfe:146-148)
__global__ __launch_bounds__(256) void k_fb_keypoints_out(const FbBlock* __restrict__ D, const float4* __restrict__ dsg, const int* __restrict__ kpg, int K,
                                                          float* __restrict__ lcs) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= K) return;
  const int b = fb_find(D->koff, D->nb, t), j = t - D->koff[b];
  const int id = kpg[D->coff[b] + j];
  const float4 P = dsg[D->moff[b] + id];
  const FbCloud& C = D->c[b];
  C.kp[j] = id;
  C.kpx[(size_t)j * 3] = (double)P.x; C.kpx[(size_t)j * 3 + 1] = (double)P.y; C.kpx[(size_t)j * 3 + 2] = (double)P.z;
  if (lcs) { lcs[(size_t)t * 12 + 9] = P.x; lcs[(size_t)t * 12 + 10] = P.y; lcs[(size_t)t * 12 + 11] = P.z; }
}

__global__ __launch_bounds__(256) void k_fb_zero_feat(const FbBlock* __restrict__ D, int K) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= K * 56) return;
  const int q = t / 56, r = t % 56, v = r / 14, w = r % 14;
  const int b = fb_find(D->koff, D->nb, q), j = q - D->koff[b], kb = D->koff[b + 1] - D->koff[b];
  reinterpret_cast<unsigned*>(D->c[b].feat)[((size_t)v * kb + j) * 14 + w] = 0u;
}

// keyfpfh (fpfh.hpp:93-115): the histogram rows of every cloud's keypoints into the cloud handle
__global__ __launch_bounds__(256) void k_fb_gather_rows33(const FbBlock* __restrict__ D, const float* __restrict__ hist, int K) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= K * 33) return;
  const int q = t / 33, r = t % 33;
  const int b = fb_find(D->koff, D->nb, q), j = q - D->koff[b];
  reinterpret_cast<float*>(D->c[b].feat)[(size_t)j * 33 + r] = hist[((size_t)D->moff[b] + D->c[b].kp[j]) * 33 + r];
}

__global__ __launch_bounds__(BT) void k_fb_bsc(const FbBlock* __restrict__ D, const float4* __restrict__ pts, const unsigned* __restrict__ start, BscConst C,
                                               float* __restrict__ lcs) {
  const int q = blockIdx.x;
  const int b = fb_find(D->koff, D->nb, q);
  GridArgs G;
  G.d = D->g2[b]; G.pts = pts; G.start = start + D->cb2[b];
  gh_bsc_keypoint(G, C, q - D->koff[b], D->koff[b + 1] - D->koff[b], D->c[b].feat, lcs + (size_t)D->koff[b] * 12);
}

// one grid of the batch: global cell keys -> stable sort -> points in cell order -> cell table
int build_grid(ghicp_ctx* ctx, const FbBlock* D, const FbBlock* H, int which, const float4* dsg, int M, unsigned total_cells, const GridSlots& sl,
               const float4** pts_out, const unsigned** start_out, const unsigned** keys_out) {
  hipStream_t s = ctx->stream;
  GridBufs B;
  GH_TRY(gh_grid_reserve(ctx, sl, (size_t)M, total_cells, true, &B));
  hipEvent_t kg = ctx->kt_begin(KT_FB_GRID);
  // stable: a cell keeps its points in down-sampled order (prims.hip).  The down-sampled clouds are the sort's segments: a cloud's points are
  // sorted on the cell inside the cloud's own grid (key - cell base), so the bits are those of the largest grid, not of all grids together.
  // The key kernel runs over the sort's tiles and leaves the first place's counts where the sort wants them.
  int cell_bits = 0;
  for (int b = 0; b < H->nb; b++) {
    const unsigned ncell = which ? H->g2[b].ncell : H->g1[b].ncell;
    if (H->moff[b + 1] > H->moff[b] && ncell > 1) cell_bits = std::max(cell_bits, bits_for(ncell - 1));
  }
  GhRsSort R;
  GH_TRY(gh_rs_seg_begin(ctx, H->nb, H->moff, cell_bits, 0, &R));
  if (ctx->sort_trace) fprintf(stderr, "sort_trace grid%d clouds=%d keys=%d bits_one_grid=%d bits_all_grids=%d places=%d\n", which + 1, H->nb, M, cell_bits, bits_for(total_cells), R.P.places);
  if (!ctx->sort_segments) R.first.table = nullptr;
  hipLaunchKernelGGL(k_fb_cell_keys, dim3(R.S.toff[R.S.nseg]), dim3(256), 0, s, D, which, dsg, R.S, B.keys, B.vals, R.first);
  R.have_first = R.first.table != nullptr;
  if (ctx->sort_segments) GH_TRY(gh_radix_sort_seg_u32(ctx, B.keys, B.keys2, B.vals, B.vals2, R, which ? D->cb2 : D->cb1, 0));
  else GH_TRY(gh_radix_sort_u32(ctx, B.keys, B.keys2, B.vals, B.vals2, M, 0, bits_for(total_cells)));
  hipLaunchKernelGGL(k_gather_sorted_f4, dim3(cdiv(M, 256)), dim3(256), 0, s, dsg, (const unsigned*)B.vals2, M, B.pts);  // w = index into the concatenated cloud
  gh_cell_start_launch(s, B.keys2, (unsigned)M, total_cells, B.start);  // (round 5: the table is filled from the sorted keys, grid.hip)
  ctx->kt_end(KT_FB_GRID, kg);
  GH_HIP(hipGetLastError());
  *pts_out = B.pts; *start_out = B.start; *keys_out = B.keys2;
  return GHICP_OK;
}

int fb_cloud_by_cloud(int n_clouds, ghicp_cloud* const* clouds, const float* const* xyz, const int64_t* n, int stride) {
  for (int i = 0; i < n_clouds; i++) GH_TRY(ghicp_cloud_recompute(clouds[i], xyz[i], n[i], stride));
  return GHICP_OK;
}

// two batches of half the clouds (a single cloud always fits: n < 2^31 - 2, and gh_grid_desc limits it to 2^26 cells per grid)
int fb_halve(ghicp_ctx* ctx, int n_clouds, ghicp_cloud* const* clouds, const float* const* xyz, const int64_t* n, int stride) {
  if (n_clouds == 1) return ghicp_cloud_recompute(clouds[0], xyz[0], n[0], stride);
  const int half = n_clouds / 2;
  GH_TRY(ghicp_clouds_recompute(ctx, half, clouds, xyz, n, stride));
  return ghicp_clouds_recompute(ctx, n_clouds - half, clouds + half, xyz + half, n + half, stride);
}

}  // namespace

// pinned mirror of the descriptor block and of the report, their device block; the handles reset, the raw clouds described
int FbRun::begin(const float* const* xyz, const int64_t* n, int stride) {
  if (!ctx->fb_pinned) {
    if (hipHostMalloc(&ctx->fb_pinned, sizeof(FbBlock) + sizeof(FbOut) + 256, hipHostMallocDefault) != hipSuccess)
      return ctx->fail(GHICP_ERR_HIP, "ghicp_clouds_recompute: pinned allocation failed");
  }
  H = reinterpret_cast<FbBlock*>(ctx->fb_pinned);
  HO = reinterpret_cast<FbOut*>(reinterpret_cast<char*>(ctx->fb_pinned) + ((sizeof(FbBlock) + 63) / 64) * 64);
  char* dblock;
  GH_TRY(ctx->reserve(B_FB_DESC, sizeof(FbBlock) + sizeof(FbOut) + 256, &dblock));
  D = reinterpret_cast<FbBlock*>(dblock);
  O = reinterpret_cast<FbOut*>(dblock + ((sizeof(FbBlock) + 63) / 64) * 64);
  memset(H, 0, sizeof(FbBlock));
  H->nb = nb;
  for (int b = 0; b < nb; b++) {
    ghicp_cloud* c = clouds[b];
    c->n = n[b]; c->m = 0; c->k = 0; c->cand = 0; c->bbx = 0.f;
    c->rf_invalidate();
    c->gc_invalidate();
    c->ov_invalidate();
    c->V = cfg.reg.dof > 4 ? 4 : (cfg.reg.dof > 0 ? 2 : 1);
    H->c[b].xyz = xyz[b]; H->c[b].n = (int)n[b]; H->c[b].stride = stride;
    H->roff[b + 1] = H->roff[b] + (int)n[b];
  }
  return GHICP_OK;
}

// ------------------------------------------------------------------ boxes of the raw clouds, voxel multipliers          (sync 1)
int FbRun::raw_boxes() {
  GH_HIP(upload());
  hipLaunchKernelGGL(k_box_init, dim3(cdiv(nb * 6, 256)), dim3(256), 0, s, O->bb, nb * 6);
  hipLaunchKernelGGL(k_fb_bbox, dim3(64, nb), dim3(256), 0, s, (const FbBlock*)D, (const float*)nullptr, 0, O->bb);
  GH_HIP(report());
  ebmax = 1;
  for (int b = 0; b < nb; b++) {
    FbCloud& C = H->c[b];
    if (C.n == 0) continue;
    float mm[6];
    gh_box_decode(HO->bb + b * 6, mm);
    C.vinv = 1.0f / cfg.voxel;  // filter.hpp:30
    unsigned long long maxv[3];
    for (int d = 0; d < 3; d++) {
      C.vmn[d] = mm[d];
      const float gap = mm[3 + d] - mm[d];
      maxv[d] = (unsigned long long)(std::ceil(gap * C.vinv) + 1);  // filter.hpp:38-40
    }
    C.mul_x = maxv[1] * maxv[2];
    C.mul_y = maxv[2];
    const long double total = (long double)maxv[0] * (long double)maxv[1] * (long double)maxv[2];
    if (total >= 18446744073709551615.0L) return ctx->fail(GHICP_ERR_CAPACITY, "voxel filter: the number of boxes exceeds the limit");  // filter.hpp:42-46
    ebmax = std::max(ebmax, bits_for((maxv[0] - 1) * C.mul_x + (maxv[1] - 1) * C.mul_y + (maxv[2] - 1)));
  }
  cloud_bits = nb > 1 ? bits_for((unsigned long long)nb - 1) : 0;
  return ebmax + cloud_bits > 64 ? FB_CLOUD_BY_CLOUD : GHICP_OK;  // no room for the cloud id above the voxel key
}

// ------------------------------------------------------------------ voxel filter, down-sampled clouds, their boxes    (sync 2)
int FbRun::voxel() {
  unsigned long long *vkeys, *vkeys2;
  unsigned *vvals, *vvals2;
  int* headpos;
  GH_TRY(ctx->reserve(B_GRID_KEYS, (size_t)N * 2 + 2, (unsigned**)&vkeys));
  GH_TRY(ctx->reserve(B_GRID_KEYS2, (size_t)N * 2 + 2, (unsigned**)&vkeys2));
  GH_TRY(ctx->reserve(B_GRID_VALS, (size_t)N + 1, &vvals));
  GH_TRY(ctx->reserve(B_GRID_VALS2, (size_t)N + 1, &vvals2));
  GH_TRY(ctx->reserve(B_FE_FLAGS, (size_t)N + nb + 16, &flags));  // also the prune flags of the M <= N + nb down-sampled rows (a phantom row per cloud)
  GH_TRY(ctx->reserve(B_FB_HEADPOS, (size_t)N + 1, &headpos));
  GH_TRY(ctx->reserve(B_FE_SCAN, 16, &misc));
  GH_TRY(ctx->reserve(B_FB_DS, (size_t)N + nb + 1, &dsg));
  GH_HIP(upload());
  hipEvent_t kv0 = ctx->kt_begin(KT_FB_VOXEL);
  // index bits: enough for the N concatenated points; packed when key and index fit 64 bits together (always at TLS sizes: 34 + 25)
  int idx_bits = 1;
  while ((1ll << idx_bits) < N) idx_bits++;
  if (ebmax + cloud_bits + idx_bits > 64) idx_bits = 0;
  // the raw clouds are the sort's segments: a cloud's points are sorted among themselves on the voxel key's bits alone, the id above them rides
  // along; the key kernel runs over the sort's tiles and leaves the first place's counts where the sort wants them
  GhRsSort R;
  GH_TRY(gh_rs_seg_begin(ctx, nb, H->roff, ebmax, 0, &R));
  if (ctx->sort_trace) fprintf(stderr, "sort_trace voxel clouds=%d keys=%lld voxel_bits=%d cloud_id_bits=%d places=%d\n", nb, N, ebmax, cloud_bits, R.P.places);
  if (!ctx->sort_segments) R.first.table = nullptr;
  hipLaunchKernelGGL(k_fb_voxel_keys, dim3(R.S.toff[R.S.nseg]), dim3(256), 0, s, (const FbBlock*)D, R.S, ebmax, idx_bits, vkeys, vvals, R.first);
  R.have_first = R.first.table != nullptr;
  ctx->kt_end(KT_FB_VOXEL, kv0);
  const int sort_bits = ebmax + cloud_bits;
  hipEvent_t kev = ctx->kt_begin(KT_VOXEL_SORT);
  // stable: lowest index leads its voxel (prims.hip)
  if (ctx->sort_segments && idx_bits > 0) GH_TRY(gh_radix_sort_seg_u64(ctx, vkeys, vkeys2, nullptr, nullptr, R, idx_bits));
  else if (ctx->sort_segments) GH_TRY(gh_radix_sort_seg_u64(ctx, vkeys, vkeys2, vvals, vvals2, R, 0));
  else if (idx_bits > 0) GH_TRY(gh_radix_sort_u64(ctx, vkeys, vkeys2, nullptr, nullptr, N, idx_bits, idx_bits + sort_bits));
  else GH_TRY(gh_radix_sort_u64(ctx, vkeys, vkeys2, vvals, vvals2, N, 0, sort_bits));
  ctx->kt_end(KT_VOXEL_SORT, kev);
  const unsigned long long vmask = ebmax >= 64 ? ~0ull : ((1ull << ebmax) - 1ull);
  hipEvent_t kv1 = ctx->kt_begin(KT_FB_VOXEL);
  hipLaunchKernelGGL(k_fb_voxel_flags, dim3(cdiv(N, 256)), dim3(256), 0, s, vkeys2, (int)N, vmask, idx_bits, flags);
  GH_TRY(gh_select_flagged_iota(ctx, flags, N, headpos, misc));  // positions of the run heads, ascending (prims.hip)
  hipLaunchKernelGGL(k_fb_voxel_bounds, dim3(1), dim3(128), 0, s, headpos, misc, D, O);
  hipLaunchKernelGGL(k_fb_gather_ds, dim3(cdiv(N + nb, 256)), dim3(256), 0, s, (const FbBlock*)D, headpos, vvals2,
                     idx_bits > 0 ? (const unsigned long long*)vkeys2 : (const unsigned long long*)nullptr, idx_bits > 0 ? (1ull << idx_bits) - 1ull : 0ull, dsg);
  hipLaunchKernelGGL(k_box_init, dim3(cdiv(nb * 6, 256)), dim3(256), 0, s, O->bb, nb * 6);
  hipLaunchKernelGGL(k_fb_bbox, dim3(64, nb), dim3(256), 0, s, (const FbBlock*)D, reinterpret_cast<const float*>(dsg), 1, O->bb);
  ctx->kt_end(KT_FB_VOXEL, kv1);
  GH_HIP(hipGetLastError());
  GH_HIP(report());
  return GHICP_OK;
}

// ------------------------------------------------------------------ the three grids of every cloud, their cell bases   (host only)
int FbRun::plan_grids(BscConst* BC) {
  const float r_pca = cfg.neighborhood_radius, r_nms = cfg.reg.radius_nonmax;
  float r_search = 0.f;
  if (bsc) GH_TRY(gh_bsc_make_const(ctx, r_nms, cfg.reg.dof, cfg.pattern, BC, &r_search));
  t1 = t2 = t3 = 0;
  for (int b = 0; b <= nb; b++) { H->hoff[b] = HO->hoff[b]; H->moff[b] = HO->moff[b]; }
  M = H->moff[nb];
  for (int b = 0; b < nb; b++) {
    ghicp_cloud* c = clouds[b];
    c->m = H->moff[b + 1] - H->moff[b];
    float mm[6] = {0, 0, 0, 0, 0, 0};
    if (c->m > 0) gh_box_decode(HO->bb + b * 6, mm);
    c->bbx = (float)((double)mm[3] - (double)mm[0] + (double)mm[4] - (double)mm[1] + (double)mm[5] - (double)mm[2]);  // main:91-93
    H->g1[b] = gh_grid_desc(mm, c->m, r_pca * 1.0001f);
    H->cb1[b] = (unsigned)t1;
    t1 += H->g1[b].ncell;
    // the NMS grid (cell side R): over the box of the DOWN-SAMPLED cloud, which the host holds already -- the candidates lie inside
    // (rounds 2-5 reduced the candidates' own box and synchronised once more to read it)
    H->g3[b] = gh_grid_desc(mm, c->m, r_nms * 1.0001f);
    H->hb[b] = (unsigned)t3;
    if (c->m > 0) t3 += H->g3[b].ncell;
    if (bsc || fpfh) {  // the feature's grid: sqrt(3) R search of the BSC encoder, or the kNN grid of the FPFH estimation
      H->g2[b] = gh_grid_desc(mm, c->m, bsc ? r_search * 1.0001f : gh_fpfh_cell(mm, c->m));
      H->cb2[b] = (unsigned)t2;
      t2 += H->g2[b].ncell;
    }
  }
  H->cb1[nb] = (unsigned)t1; H->cb2[nb] = (unsigned)t2; H->hb[nb] = (unsigned)t3;
  // the cell tables of all clouds are summed into one: when that gets large (clouds of large extent), halve the batch instead of
  // failing -- whatever the cloud-by-cloud path handles must work here too
  constexpr unsigned long long FB_CELL_BUDGET = 1ull << 28;  // 1 GB of cell table per grid
  return (t1 >= FB_CELL_BUDGET || t2 >= FB_CELL_BUDGET || t3 >= FB_CELL_BUDGET) ? FB_HALVE : GHICP_OK;
}

// ------------------------------------------------------------------ PCA grid, PCA, prune                              (sync 3)
int FbRun::pca_prune() {
  float* lambda;
  int* count;
  unsigned* cells;
  GH_TRY(ctx->reserve(B_FE_LAMBDA, (size_t)M * 3 + 3, &lambda));
  GH_TRY(ctx->reserve(B_FE_CURV, (size_t)M + 1, &curv));
  GH_TRY(ctx->reserve(B_FE_COUNT, (size_t)M + 1, &count));
  GH_TRY(ctx->reserve(B_FE_CAND, (size_t)M + 1, &cand));
  GH_TRY(ctx->reserve(B_FE_SORTK, (size_t)M * 2 + 2, &cells));
  GH_HIP(upload());
  const float4* pts1;
  const unsigned *start1, *keys1;
  const GridSlots sl1 = {B_GRID_KEYS, B_GRID_KEYS2, B_GRID_VALS, B_GRID_VALS2, B_GRID_START, B_GRID_PTS};
  GH_TRY(build_grid(ctx, D, H, 0, dsg, M, (unsigned)t1, sl1, &pts1, &start1, &keys1));
  hipEvent_t ku = ctx->kt_begin(KT_FB_GRID);
  GH_TRY(gh_unique_sorted_u32(ctx, keys1, M, cells, misc));  // the occupied cells, ascending (prims.hip)
  GH_HIP(hipMemsetAsync(misc + 4, 0, 8 * sizeof(int), s));
  ctx->kt_end(KT_FB_GRID, ku);
  const float r_pca = cfg.neighborhood_radius, r2_pca = (float)((double)r_pca * (double)r_pca);  // pcl radiusSearch: static_cast<float>(radius*radius)
  hipEvent_t kt = ctx->kt_begin(KT_PCA);
  double* scat;
  GH_TRY(ctx->reserve(B_FE_SCATTER, (size_t)M * 6 + 6, &scat));
  int pca_per_cu = 0;  // every workgroup of the launch resident at once: the runs are handed out dynamically, a second round of workgroups would only find the counters dry
  GH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pca_per_cu, reinterpret_cast<const void*>(&k_fb_pca_cells<PCA_CHUNK>), 64, 0));
  const int pca_blocks = std::max(8, (std::max(1, std::min(pca_per_cu, 20)) * ctx->num_cu) & ~7);
  hipLaunchKernelGGL(k_fb_pca_cells<PCA_CHUNK>, dim3(pca_blocks), dim3(64), 0, s, (const FbBlock*)D, pts1, start1, (const unsigned*)cells,
                     (const int*)misc, misc + 4, r2_pca, scat, count);
  hipLaunchKernelGGL(k_fb_pca_eigen, dim3(cdiv(M, 256)), dim3(256), 0, s, (const double*)scat, (const int*)count, M, lambda, curv);
  ctx->kt_end(KT_PCA, kt);
  hipEvent_t kp = ctx->kt_begin(KT_FB_PRUNE);
  hipLaunchKernelGGL(k_fb_prune_flags, dim3(cdiv(M, 256)), dim3(256), 0, s, lambda, count, M, cfg.ratio_max, cfg.min_neighbors, flags);
  GH_TRY(gh_select_flagged_iota(ctx, flags, M, cand, misc + 2));  // the candidates' point indices, ascending (prims.hip)
  hipLaunchKernelGGL(k_fb_cand_bounds, dim3(1), dim3(128), 0, s, (const int*)cand, (const int*)(misc + 2), D, O);
  ctx->kt_end(KT_FB_PRUNE, kp);
  GH_HIP(hipGetLastError());
  GH_HIP(report());
  for (int b = 0; b <= nb; b++) H->coff[b] = HO->coff[b];
  for (int b = 0; b < nb; b++) clouds[b]->cand = H->coff[b + 1] - H->coff[b];
  Ctot = H->coff[nb];
  return GHICP_OK;
}

// ------------------------------------------------------------------ outputs into the handles
int FbRun::outputs() {
  for (int b = 0; b < nb; b++) {
    ghicp_cloud* c = clouds[b];
    GH_HIP(c->ds.reserve(((size_t)c->m + 1) * sizeof(float4)));
    GH_HIP(c->kp.reserve(((size_t)c->m + 1) * sizeof(int)));
    GH_HIP(c->kpx.reserve(((size_t)c->k * 3 + 3) * sizeof(double)));
    if (bsc) GH_HIP(c->feat.reserve((size_t)4 * c->k * 56 + 64));
    if (fpfh) GH_HIP(c->feat.reserve(((size_t)c->k * 33 + 33) * sizeof(float)));
    H->c[b].ds = c->ds.as<float4>(); H->c[b].kp = c->kp.as<int>(); H->c[b].kpx = c->kpx.as<double>(); H->c[b].feat = c->feat.as<uint8_t>();
  }
  GH_HIP(upload());
  hipEvent_t ko = ctx->kt_begin(KT_FB_OUT);
  hipLaunchKernelGGL(k_fb_copy_ds, dim3(cdiv(M, 256)), dim3(256), 0, s, (const FbBlock*)D, (const float4*)dsg, M);
  lcs = nullptr;
  if (Ktot > 0) {
    if (bsc) GH_TRY(ctx->reserve(B_P_LCS, (size_t)Ktot * 12 + 12, &lcs));
    hipLaunchKernelGGL(k_fb_keypoints_out, dim3(cdiv(Ktot, 256)), dim3(256), 0, s, (const FbBlock*)D, (const float4*)dsg, (const int*)kpg, Ktot, lcs);
    if (bsc) hipLaunchKernelGGL(k_fb_zero_feat, dim3(cdiv((long long)Ktot * 56, 256)), dim3(256), 0, s, (const FbBlock*)D, Ktot);
  }
  ctx->kt_end(KT_FB_OUT, ko);
  return GHICP_OK;
}

// ------------------------------------------------------------------ feature grid; BSC strings or FPFH rows            (last sync)
int FbRun::features(const BscConst& BC) {
  if (Ktot > 0 && (bsc || fpfh)) {
    const float4* pts2;
    const unsigned *start2, *keys2;
    const GridSlots sl2 = {B_GRID2_KEYS, B_GRID2_KEYS2, B_GRID2_VALS, B_GRID2_VALS2, B_GRID2_START, B_GRID2_PTS};
    GH_TRY(build_grid(ctx, D, H, 1, dsg, M, (unsigned)t2, sl2, &pts2, &start2, &keys2));
    if (bsc) {
      hipEvent_t kb = ctx->kt_begin(KT_BSC);
      hipLaunchKernelGGL(k_fb_bsc, dim3((unsigned)Ktot), dim3(BT), 0, s, (const FbBlock*)D, pts2, start2, BC, lcs);
      ctx->kt_end(KT_BSC, kb);
    } else {  // compute_fpfh_feature over ALL down-sampled points, then the keypoints' rows (main:122-127)
      float* hist;
      GH_TRY(ctx->reserve(B_P_FEAT_S, (size_t)M * 33 * sizeof(float) + 64, (char**)&hist));
      GH_TRY(gh_fpfh_batch_dev(ctx, dsg, M, pts2, start2, D->g2, D->cb2, D->moff, nb, hist));
      hipLaunchKernelGGL(k_fb_gather_rows33, dim3(cdiv((long long)Ktot * 33, 256)), dim3(256), 0, s, (const FbBlock*)D, (const float*)hist, Ktot);
    }
  }
  GH_HIP(hipGetLastError());
  GH_HIP(hipStreamSynchronize(s));
  return GHICP_OK;
}

// Front ends of n_clouds raw clouds (device pointers xyz[i], n[i] points of `stride` floats) into existing handles of ONE front-end
// configuration and one context.  Equivalent to ghicp_cloud_recompute(clouds[i], xyz[i], n[i], stride) for every i, bit for bit.
extern "C" int ghicp_clouds_recompute(ghicp_ctx* ctx, int32_t n_clouds, ghicp_cloud* const* clouds, const float* const* xyz, const int64_t* n, int stride) {
  GH_ENTER(ctx);
  GH_ARG(n_clouds >= 0 && (n_clouds == 0 || (clouds != nullptr && xyz != nullptr && n != nullptr)) && stride >= 3);
  if (n_clouds == 0) return GHICP_OK;
  FbRun R;
  R.ctx = ctx; R.s = ctx->stream; R.nb = n_clouds; R.clouds = clouds; R.N = 0;
  for (int i = 0; i < n_clouds; i++) {
    GH_ARG(clouds[i] != nullptr && clouds[i]->ctx == ctx && n[i] >= 0 && n[i] < (1ll << 31) - 2);
    if (!same_front_end(clouds[i]->cfg, clouds[0]->cfg))
      return ctx->fail(GHICP_ERR_ARG, "ghicp_clouds_recompute: cloud %d has a different front-end configuration", i);
    for (int j = 0; j < i; j++) GH_ARG(clouds[j] != clouds[i]);
    R.N += n[i];
  }
  R.cfg = clouds[0]->cfg; R.bsc = R.cfg.reg.feature == GHICP_FEATURE_BSC; R.fpfh = R.cfg.reg.feature == GHICP_FEATURE_FPFH;
  // what the batch does not cover goes cloud by cloud: no down-sampling, host pointers
  if (!(R.cfg.voxel > 0.f) || ctx->host_ptrs) return fb_cloud_by_cloud(n_clouds, clouds, xyz, n, stride);
  if (n_clouds > FB_MAX || R.N + n_clouds >= (1ll << 31) - 2) return fb_halve(ctx, n_clouds, clouds, xyz, n, stride);
  GH_TRY(R.begin(xyz, n, stride));
  if (R.N == 0) return GHICP_OK;
  BscConst BC;
  int rc = R.raw_boxes();
  if (rc == GHICP_OK) rc = R.voxel();
  if (rc == GHICP_OK) rc = R.plan_grids(&BC);
  if (rc == FB_CLOUD_BY_CLOUD) return fb_cloud_by_cloud(n_clouds, clouds, xyz, n, stride);
  if (rc == FB_HALVE) return fb_halve(ctx, n_clouds, clouds, xyz, n, stride);
  if (rc != GHICP_OK || R.M <= 0) return rc;
  GH_TRY(R.pca_prune());
  GH_TRY(R.nms());
  GH_TRY(R.outputs());
  return R.features(BC);
}
