// Internal: what the stages of the batched front end (batch.hip) and its round-based NMS (batch_nms.hip) share -- the descriptor block the kernels
// look their cloud up in, the report the device sends back, and the host-side state of a batch in flight (FbRun).
#pragma once
#include "cloud.h"
#include "devmath.h"

constexpr int FB_MAX = 64;  // clouds per batch
constexpr int FB_NMS_ROUNDS = 16;  // NMS rounds per launch sequence (the host looks at the last one's count and launches another sequence if need be)

struct FbCloud {
  const float* xyz;  // raw cloud
  int n, stride;
  float vmn[3], vinv;              // voxel filter (filter.hpp:28-40)
  unsigned long long mul_x, mul_y;
  float4* ds;                      // outputs: the cloud handle's buffers
  int* kp;
  double* kpx;
  uint8_t* feat;
};

// Host -> device descriptor block (uploaded once per stage) ...
struct FbBlock {
  FbCloud c[FB_MAX];
  GridDesc g1[FB_MAX], g2[FB_MAX], g3[FB_MAX];  // PCA grid, BSC grid, NMS grid of selected keypoints
  int roff[FB_MAX + 1];                         // raw points
  int hoff[FB_MAX + 1];                         // voxel run heads (device written)
  int moff[FB_MAX + 1];                         // down-sampled points (device written)
  int coff[FB_MAX + 1];                         // NMS candidates (device written)
  int koff[FB_MAX + 1];                         // keypoints
  unsigned cb1[FB_MAX + 1], cb2[FB_MAX + 1], hb[FB_MAX + 1];  // cell bases of the three grids
  int nb, pad_;
};
// ... and what the device reports back
struct FbOut {
  int bb[FB_MAX * 6];
  int hoff[FB_MAX + 1], moff[FB_MAX + 1], coff[FB_MAX + 1];
  int kcount[FB_MAX];
  int nms_und[FB_NMS_ROUNDS];  // candidates each NMS round of the last sequence left undecided
};

// largest b in [0, nb) with off[b] <= i (off ascending; clouds without items are skipped over)
template <typename T>
__device__ inline int fb_find(const T* __restrict__ off, int nb, T i) {
  int lo = 0, hi = nb - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ inline unsigned long long fb_f64_key(double v) {  // order-preserving f64 -> u64, -0.0 keyed as +0.0 (nms.hip)
  const unsigned long long b = v == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// One batch in flight, host side: what a stage of ghicp_clouds_recompute leaves for the stages after it
struct BscConst;
struct FbRun {
  ghicp_ctx* ctx;
  hipStream_t s;
  ghicp_pair_config cfg;
  bool bsc, fpfh;  // the configuration's feature
  int nb;
  ghicp_cloud* const* clouds;
  FbBlock *H, *D;  // the descriptor block: pinned mirror, device
  FbOut *HO, *O;   // the report: pinned mirror, device
  long long N;     // raw points of the batch
  int ebmax, cloud_bits;          // bits of the widest voxel key, of the cloud id above it
  int M, Ctot, Ktot;              // down-sampled points, NMS candidates, keypoints of the batch
  unsigned long long t1, t2, t3;  // cells of the batch's PCA grid, feature grid, NMS grid
  float4* dsg;                    // concatenated down-sampled clouds
  unsigned char* flags;           // voxel run heads, then the prune flags
  int* misc;                      // totals of the selects and of the unique, the PCA kernel's run counters
  double* curv;
  int *cand, *kpg;  // candidate -> global point index, ascending; per cloud (at coff[b]) the keypoint ids into the cloud, in rank order
  float* lcs;       // BSC: the keypoints' local coordinate systems
  hipError_t upload() { return hipMemcpyAsync(D, H, sizeof(FbBlock), hipMemcpyHostToDevice, s); }
  hipError_t report() {  // a host synchronisation
    hipError_t e = hipMemcpyAsync(HO, O, sizeof(FbOut), hipMemcpyDeviceToHost, s);
    return e != hipSuccess ? e : hipStreamSynchronize(s);
  }
  // the stages in the order they run (batch.hip; nms: batch_nms.hip); raw_boxes and plan_grids may find the batch not covered
  int begin(const float* const* xyz, const int64_t* n, int stride), raw_boxes(), voxel(), plan_grids(BscConst* BC), pca_prune(), nms(), outputs(), features(const BscConst& BC);
};
