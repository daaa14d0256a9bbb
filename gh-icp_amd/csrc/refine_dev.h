// Internal: what the driver of the batched fine registration (refine.hip) shares with the reciprocal stage of its loop (refine_recip.hip) --
// the pair descriptors and the per-chunk arrays every k_rf_* / k_rr_* kernel receives by value.
#pragma once
#include "icp_dev.h"
#include "refine_recip_plan.h"

namespace rfdev {

struct RefinePair {
  icpdev::NnIndex X;  // the target's grids (buffers of its handle)
  const float4* tgt;  // the target's down-sampled points
  const float* tnrm;  // its normals (point-to-plane)
  const float4* src;  // the source's down-sampled points
  long long off;      // the pair's slice of the concatenated per-point arrays
  int ns, pad_;
  float init[16];     // float(Rt_init)
};

struct RefineArgs {
  const RefinePair* pair;
  icpdev::IcpState* st;
  float4* cur;
  int* nn;
  float* nd;
  unsigned* pend;      // work lists of the coarse search, one slice per pair
  unsigned* pendc;     // their lengths
  unsigned* ovl;       // calOverlap counts
  double* part;        // NBLK x NPART per pair
  unsigned* hist;      // 6 x SEL_BINS per pair
  unsigned char* flag; // 1: the pair is frozen
};

constexpr int COARSE_BLK = 512;  // blocks per pair of the coarse search (any count gives the same result: one wave per query)

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
