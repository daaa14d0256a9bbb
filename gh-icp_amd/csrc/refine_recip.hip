// Reciprocal correspondences inside the batched fine registration over cached clouds (ghicp_refine_clouds_reciprocal; the driver is refine.hip):
// pcl's determineReciprocalCorrespondences as ghicp_icp runs it (icp.hip: build_index over the moved source, k_gather_query, nn_search,
// k_reciprocal) for EVERY running pair of a chunk in one launch sequence per iteration, with no host wait.
//
// Why any grid will do.  nn_fine_body / nn_coarse_body are exact 1-NN searches with ties to the lower index, and the index travels in pts.w:
// the result does not depend on the grid's cell, origin or dimensions.  So a pair need not get the grids gh_grid_build would give its moved
// source (their size is known only after a host read of the bounding box); it gets grids that fit a range of ONE cell table sized before
// the loop, and its back-search still returns what ghicp_icp's returns, bit for bit.  The search runs in the moved source's frame on the
// moved points themselves -- the same float distances, the same ties -- and w holds the index WITHIN the pair, so the test back == i reads
// as in k_reciprocal.
//
// Per iteration (gh_refine_recip_step), after the forward search:
//   k_box_init, k_rr_box      per-pair bounding box of the pair's slice of cur: 2-D launch, then the block tail every box reduction shares
//                             (gh_box_block, grid.h: wave shuffles, 4 waves through LDS, six ordered-int atomicMin / atomicMax per block)
//   k_rr_plan                 one thread per pair: its fine grid (from the target's fine cell) and its coarse grid (8 x the fine cell that came
//                             out) inside the pair's ranges of the table -- gh_recip_grid (refine_recip_plan.h: the budget rule is written there)
//   k_rr_keys                 every point twice: key = base_f[p] + fine cell in the first half, base_c[p] + coarse cell in the second
//   gh_radix_sort_u32         ONE sort over both halves, bits_for(cells of the table) bits, constant over the loop
//   k_rr_gather               points in cell order, w = index within the pair
//   gh_cell_start_launch      ONE table; a pair's grid is the table from its base on (cell starts are positions in the one sorted array)
//   k_rr_query                q[i] = tgt[max(nn[i], 0)]
//   k_rr_nn_fine / _coarse    the back-search, with work lists and counters of its own (the forward search's stay untouched)
//   k_rr_kill                 nn[i] = -1 where the back-search does not return i; nd stays
// Two grids per pair (fine + coarse), as ghicp_icp builds: a query far from the moved source (the target point an outlier chose) costs a
// bounded number of cells.  A single grid would save half the sort; the two have not been measured against each other.
// A frozen pair (icpdev::frozen) takes no part: its blocks return before the box, the plan, the query, the searches and the kill.  Its points
// ride along in the sort under the first key of the pair's own ranges, where no search looks: nothing of the pair is written.
// blockIdx.y is the pair and uniform over the block: the descriptor reads are scalar loads.  No float atomics.  These kernels spell the 2-D
// prologue out: with point_block / coarse_blocks of refine_dev.h (the forward loop's form) this stage measured 0.6 % slower.
#include "prims.h"
#include "refine_dev.h"

namespace {

using namespace icpdev;
using namespace rfdev;

__global__ __launch_bounds__(256) void k_rr_box(RefineArgs A, RecipStage R) {
  const unsigned p = blockIdx.y;
  const RefinePair& D = A.pair[p];
  if (blockIdx.x * 256u >= (unsigned)D.ns) return;
  if (frozen(&A.st[p])) return;
  const float4* cur = A.cur + D.off;
  float mn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, mx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < D.ns; i += gridDim.x * 256) {
    const float4 P = cur[i];
    mn[0] = fminf(mn[0], P.x); mx[0] = fmaxf(mx[0], P.x);
    mn[1] = fminf(mn[1], P.y); mx[1] = fmaxf(mx[1], P.y);
    mn[2] = fminf(mn[2], P.z); mx[2] = fmaxf(mx[2], P.z);
  }
  gh_box_block(mn, mx, R.box + p * 6);
}

__device__ inline GridDesc desc_of(const RecipGrid& g, int n) {
  GridDesc d;
  for (int a = 0; a < 3; a++) { d.mn[a] = g.mn[a]; d.dim[a] = g.dim[a]; }
  d.inv = g.inv;
  d.n = n;
  d.ncell = g.ncell;
  return d;
}

__global__ __launch_bounds__(64) void k_rr_plan(RefineArgs A, RecipStage R, int np) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= np || frozen(&A.st[p])) return;
  float mm[6];
  for (int k = 0; k < 6; k++) mm[k] = gh_ord_dec(R.box[p * 6 + k]);
  const RecipRange rg = R.range[p];
  const RecipGrid gf = gh_recip_grid(mm, A.pair[p].X.fine.cell, rg.cells_f);  // ghicp_icp: the target's fine cell ...
  const RecipGrid gc = gh_recip_grid(mm, (1.0f / gf.inv) * 8.0f, rg.cells_c);   // ... and 8 x the fine cell that was used
  R.grid[2 * p] = desc_of(gf, A.pair[p].ns);
  R.grid[2 * p + 1] = desc_of(gc, A.pair[p].ns);
}

__global__ __launch_bounds__(256) void k_rr_keys(RefineArgs A, RecipStage R) {
  const unsigned p = blockIdx.y;
  const RefinePair& D = A.pair[p];
  if (blockIdx.x * 256u >= (unsigned)D.ns) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= D.ns) return;
  const RecipRange rg = R.range[p];
  const long long gi = D.off + i;
  unsigned kf = rg.base_f, kc = rg.base_c;  // a frozen pair: the first cell of its own ranges
  if (!frozen(&A.st[p])) {
    const float4 P = A.cur[gi];
    kf += gh_cell_key(R.grid[2 * p], P.x, P.y, P.z);
    kc += gh_cell_key(R.grid[2 * p + 1], P.x, P.y, P.z);
  }
  R.keys[gi] = kf;
  R.keys[R.npts + gi] = kc;
  R.vals[gi] = (unsigned)gi;
  R.vals[R.npts + gi] = (unsigned)gi;
  R.lidx[gi] = (unsigned)i;
}

__global__ __launch_bounds__(256) void k_rr_gather(const float4* __restrict__ cur, RecipStage R) {
  const long long t = blockIdx.x * 256ll + threadIdx.x;
  if (t >= 2 * R.npts) return;
  const unsigned v = R.vals2[t];
  const float4 P = cur[v];
  R.pts[t] = make_float4(P.x, P.y, P.z, __uint_as_float(R.lidx[v]));
}

__global__ __launch_bounds__(256) void k_rr_query(RefineArgs A, RecipStage R) {  // k_gather_query
  const unsigned p = blockIdx.y;
  const RefinePair& D = A.pair[p];
  if (blockIdx.x * 256u >= (unsigned)D.ns) return;
  if (frozen(&A.st[p])) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < D.ns) R.q[D.off + i] = D.tgt[max(A.nn[D.off + i], 0)];
}

__device__ inline NnGrid source_grid(const RecipStage& R, unsigned p, int which) {
  const GridDesc& d = R.grid[2 * p + which];
  const RecipRange& rg = R.range[p];
  return NnGrid{d, R.pts, R.start + (which ? rg.base_c : rg.base_f), 1.0f / d.inv};
}

__global__ __launch_bounds__(256) void k_rr_nn_fine(RefineArgs A, RecipStage R) {
  const unsigned p = blockIdx.y;
  const RefinePair& D = A.pair[p];
  if (blockIdx.x * 256u >= (unsigned)D.ns) return;
  if (frozen(&A.st[p])) return;
  nn_fine_body(source_grid(R, p, 0), R.q + D.off, D.ns, blockIdx.x * 256 + threadIdx.x, R.nn2 + D.off, R.nd2 + D.off, R.pend2 + D.off, &R.pendc2[p]);
}

__global__ __launch_bounds__(256) void k_rr_nn_coarse(RefineArgs A, RecipStage R) {
  const unsigned p = blockIdx.y;
  const RefinePair& D = A.pair[p];
  const unsigned nb = (unsigned)min(cdiv_dev(D.ns, 4), COARSE_BLK);
  if (blockIdx.x >= nb) return;
  if (frozen(&A.st[p])) return;
  nn_coarse_body(source_grid(R, p, 1), R.q + D.off, R.pend2 + D.off, R.pendc2[p], blockIdx.x * 4u + (threadIdx.x >> 6), nb * 4u, R.nn2 + D.off, R.nd2 + D.off);
}

__global__ __launch_bounds__(256) void k_rr_kill(RefineArgs A, RecipStage R) {  // k_reciprocal
  const unsigned p = blockIdx.y;
  const RefinePair& D = A.pair[p];
  if (blockIdx.x * 256u >= (unsigned)D.ns) return;
  if (frozen(&A.st[p])) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < D.ns && R.nn2[D.off + i] != i) A.nn[D.off + i] = -1;
}

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace

namespace rfdev {

int gh_refine_recip_begin(ghicp_ctx* ctx, const RefinePair* hd, int np, long long npts, RecipStage* R) {
  memset(R, 0, sizeof(*R));
  std::vector<int> ns((size_t)np);
  for (int p = 0; p < np; p++) ns[(size_t)p] = hd[p].ns;
  std::vector<RecipRange> ranges((size_t)np);
  const unsigned long long total = gh_recip_ranges(np, ns.data(), ranges.data());
  R->npts = npts;
  R->total = (unsigned)total;
  R->total_f = ranges[0].base_c;
  R->sort_bits = bits_for(total);
  const size_t b_range = up16((size_t)np * sizeof(RecipRange)), b_box = up16((size_t)np * 6 * sizeof(int)), b_grid = up16((size_t)np * 2 * sizeof(GridDesc));
  char* desc;
  GH_TRY(ctx->reserve(B_RR_DESC, b_range + b_box + b_grid + (size_t)np * sizeof(unsigned), &desc));
  R->range = reinterpret_cast<const RecipRange*>(desc);
  R->box = reinterpret_cast<int*>(desc + b_range);
  R->grid = reinterpret_cast<GridDesc*>(desc + b_range + b_box);
  R->pendc2 = reinterpret_cast<unsigned*>(desc + b_range + b_box + b_grid);
  const GridSlots sl = {B_GRID2_KEYS, B_GRID2_KEYS2, B_GRID2_VALS, B_GRID2_VALS2, B_GRID2_START, B_GRID2_PTS};
  GridBufs B;
  GH_TRY(gh_grid_reserve(ctx, sl, (size_t)npts * 2, (size_t)total, true, &B));
  R->keys = B.keys; R->keys2 = B.keys2; R->vals = B.vals; R->vals2 = B.vals2; R->pts = B.pts; R->start = B.start;
  GH_TRY(ctx->reserve(B_RR_LIDX, (size_t)npts + 1, &R->lidx));
  GH_TRY(ctx->reserve(B_ICP_Q, (size_t)npts + 1, &R->q));
  GH_TRY(ctx->reserve(B_ICP_NN2, (size_t)npts + 1, &R->nn2));
  GH_TRY(ctx->reserve(B_ICP_ND2, (size_t)npts + 1, &R->nd2));
  GH_TRY(ctx->reserve(B_RR_PEND, (size_t)npts + 4, &R->pend2));
  return ctx->upload_table(ranges.data(), (size_t)np * sizeof(RecipRange), desc);
}

int gh_refine_recip_step(ghicp_ctx* ctx, const RefineArgs& A, const RecipStage& R, int np, int max_gs) {
  hipStream_t s = ctx->stream;
  const long long n2 = 2 * R.npts;
  hipEvent_t kg = ctx->kt_begin(KT_REFINE_GRID);
  hipLaunchKernelGGL(k_box_init, dim3(cdiv(np * 6ll, 256)), dim3(256), 0, s, R.box, np * 6);
  hipLaunchKernelGGL(k_rr_box, dim3(min(max_gs, 64), np), dim3(256), 0, s, A, R);
  hipLaunchKernelGGL(k_rr_plan, dim3(cdiv(np, 64)), dim3(64), 0, s, A, R, np);
  hipLaunchKernelGGL(k_rr_keys, dim3(max_gs, np), dim3(256), 0, s, A, R);
  GH_TRY(gh_radix_sort_u32(ctx, R.keys, R.keys2, R.vals, R.vals2, n2, 0, R.sort_bits));
  hipLaunchKernelGGL(k_rr_gather, dim3(cdiv(n2, 256)), dim3(256), 0, s, (const float4*)A.cur, R);
  gh_cell_start_launch(s, R.keys2, (unsigned)n2, R.total, R.start);
  ctx->kt_end(KT_REFINE_GRID, kg);
  hipLaunchKernelGGL(k_rr_query, dim3(max_gs, np), dim3(256), 0, s, A, R);
  GH_HIP(hipMemsetAsync(R.pendc2, 0, (size_t)np * sizeof(unsigned), s));
  hipLaunchKernelGGL(k_rr_nn_fine, dim3(max_gs, np), dim3(256), 0, s, A, R);
  hipLaunchKernelGGL(k_rr_nn_coarse, dim3(min(cdiv(max_gs * 256ll, 4), COARSE_BLK), np), dim3(256), 0, s, A, R);
  hipLaunchKernelGGL(k_rr_kill, dim3(max_gs, np), dim3(256), 0, s, A, R);
  GH_HIP(hipGetLastError());
  return GHICP_OK;
}

}  // namespace rfdev
