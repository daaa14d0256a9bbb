// Internal, device side: what the batched refiners over cached clouds share -- ICP (refine.hip), its reciprocal stage (refine_recip.hip) and
// generalized ICP (refine_gicp.hip).  The pair descriptor and the per-chunk arrays every k_rf_* / k_rr_* / k_gb_* kernel receives by value,
// the prologue of the 2-D launches, and the kernels that are the same for both methods (k_chunk_*: the 1-NN search, the overlap count, the
// fitness sum), as templates over the method's argument block.  The host side of a chunk is refine_run.h.
#pragma once
#include "icp_dev.h"
#include "refine_recip_plan.h"

namespace rfdev {

// One pair of a chunk: what every method needs ...
struct PairCore {
  icpdev::NnIndex X;  // the target's grids (buffers of its handle)
  const float4* tgt;  // the target's down-sampled points
  const float4* src;  // the source's down-sampled points
  long long off;      // the pair's slice of the concatenated per-point arrays
  int ns, pad_;
  float init[16];     // float(Rt_init)
};
// ... and what each method adds
struct RefinePair : PairCore {
  const float* tnrm;  // the target's normals (point-to-plane)
};
struct GicpPair : PairCore {
  const double* covT;  // the target's covariances
  const double* covS;  // the source's, in the source's own frame
};

// The arrays of a chunk
template <typename Pair, typename State>
struct ChunkArrays {
  typedef Pair pair_t;
  typedef State state_t;
  const Pair* pair;
  State* st;
  float4* cur;
  int* nn;
  float* nd;
  unsigned* pend;      // work lists of the coarse search, one slice per pair
  unsigned* pendc;     // their lengths
  unsigned* ovl;       // calOverlap counts
  double* part;        // NBLK x NPART per pair
  unsigned char* flag; // 1: the pair is frozen
};
struct RefineArgs : ChunkArrays<RefinePair, icpdev::IcpState> {
  unsigned* hist;  // 6 x SEL_BINS per pair
};
struct GicpArgs : ChunkArrays<GicpPair, icpdev::GicpState> {
  double* mahal;  // 6 per source point
};
struct GicpTrimArgs : GicpArgs {  // the trimmed loop: the kernels it shares with the untrimmed one take the GicpArgs part
  icpdev::GicpSel* sel;  // one select record per pair
  unsigned* hist;        // 6 x SEL_BINS per pair
};

constexpr int COARSE_BLK = 512;  // blocks per pair of the coarse search (any count gives the same result: one wave per query)

template <typename Args>
__device__ inline double* part_of(const Args& A, unsigned p) { return A.part + (size_t)p * icpdev::NBLK * icpdev::NPART; }

// ------------------------------------------------------------------------------------------------ the prologue of a 2-D launch
// blockIdx.y is the pair, blockIdx.x the block WITHIN the pair.  A launch serves the pairs still in their loop (not frozen) or, with
// `final` set -- the first transform, the overlap count, the output cloud and its search --, every pair that was not refused.  A block past
// its pair's own count, or of a pair the launch does not serve, gets false / 0 back and returns before it touches anything of the pair.
// The helpers take VALUES (ns, the address of the state): a form returning the descriptor or nullptr loaded ns twice per block, one taking
// the argument block and the descriptor by reference turned the search kernels' reads into flat loads.
template <typename State>
__device__ inline bool left_out(const State* st, int final) { return final ? st->refused != 0 : icpdev::frozen(st); }

// per point: cdiv(ns, 256) blocks per pair.  true: this block has work
template <typename State>
__device__ inline bool point_block(int ns, const State* st, int final = 0) {
  if (blockIdx.x * 256u >= (unsigned)ns) return false;
  return !left_out(st, final);
}

// the coarse search: nb = min(cdiv(ns, 4), COARSE_BLK) blocks per pair, one wave per query.  nb, or 0
template <typename State>
__device__ inline unsigned coarse_blocks(int ns, const State* st, int final = 0) {
  const unsigned nb = (unsigned)min(cdiv_dev(ns, 4), COARSE_BLK);
  if (blockIdx.x >= nb) return 0u;
  return left_out(st, final) ? 0u : nb;
}

// ------------------------------------------------------------------------------------------------ the kernels both methods launch
template <typename Args>
__global__ __launch_bounds__(256) void k_chunk_nn_fine(Args A, int final) {
  const auto& D = A.pair[blockIdx.y];
  if (!point_block(D.ns, &A.st[blockIdx.y], final)) return;
  icpdev::nn_fine_body(D.X.fine, A.cur + D.off, D.ns, blockIdx.x * 256 + threadIdx.x, A.nn + D.off, A.nd + D.off, A.pend + D.off, &A.pendc[blockIdx.y]);
}

template <typename Args>
__global__ __launch_bounds__(256) void k_chunk_nn_coarse(Args A, int final) {
  const auto& D = A.pair[blockIdx.y];
  const unsigned nb = coarse_blocks(D.ns, &A.st[blockIdx.y], final);
  if (!nb) return;
  icpdev::nn_coarse_body(D.X.coarse, A.cur + D.off, A.pend + D.off, A.pendc[blockIdx.y], blockIdx.x * 4u + (threadIdx.x >> 6), nb * 4u, A.nn + D.off, A.nd + D.off);
}

// calOverlap from the first search: a source point (under its initial pose) counts when its nearest target point lies at d^2 < thre_dis^2
template <typename Args>
__global__ __launch_bounds__(256) void k_chunk_overlap(Args A, float r2) {
  const auto& D = A.pair[blockIdx.y];
  if (!point_block(D.ns, &A.st[blockIdx.y], 1)) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  icpdev::block_count_add(i < D.ns && A.nd[D.off + i] < r2, &A.ovl[blockIdx.y]);
}

// NBLK blocks per pair, as in the single-pair launch
template <typename Args>
__global__ __launch_bounds__(256) void k_chunk_sum(Args A) {
  const unsigned p = blockIdx.y;
  if (A.st[p].refused) return;
  const auto& D = A.pair[p];
  icpdev::sum_f32_body(A.nd + D.off, D.ns, part_of(A, p), blockIdx.x);
}

// the NBLK block sums added one after the other, as ghicp_icp and ghicp_gicp add them on the host
template <typename Args>
__global__ __launch_bounds__(64) void k_chunk_fitness(Args A, int np) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= np || A.st[p].refused) return;
  const double* part = part_of(A, (unsigned)p);
  double f = 0;
  for (int b = 0; b < icpdev::NBLK; b++) f += part[b];
  A.st[p].fit_sum = f;
}

// ------------------------------------------------------------------------------------------------ the reciprocal stage of the ICP loop
// The reciprocal test of one chunk (determineReciprocalCorrespondences): everything is reserved and planned before the loop ...
struct RecipStage {
  const RecipRange* range;         // per pair: its ranges of the cell table (refine_recip_plan.h)
  int* box;                        // per pair: 6 ordered ints (min xyz, max xyz of its moved source)
  GridDesc* grid;                  // per pair: fine, coarse -- written on the device every iteration
  unsigned *keys, *keys2, *vals, *vals2;  // 2 x npts: the fine keys of every point, then the coarse keys
  float4* pts;                     // 2 x npts points in cell order, w = index within the pair
  unsigned* start;                 // total + 1 cell starts
  unsigned* lidx;                  // npts: index of a point within its pair
  float4* q;                       // npts queries: the target point every source point chose
  int* nn2;                        // npts back-search results
  float* nd2;
  unsigned* pend2;                 // the back-search's own work lists and their lengths
  unsigned* pendc2;
  long long npts;
  unsigned total, total_f;         // cells of the table / of its fine ranges
  int sort_bits;
};
int gh_refine_recip_begin(ghicp_ctx* ctx, const RefinePair* hd, int np, long long npts, RecipStage* R);
// ... and gh_refine_recip_step puts one iteration's test of every running pair on the stream, after the forward search: no host wait
int gh_refine_recip_step(ghicp_ctx* ctx, const RefineArgs& A, const RecipStage& R, int np, int max_gs);

}  // namespace rfdev
