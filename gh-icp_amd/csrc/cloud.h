// Internal: the per-cloud front-end cache handle (cloud.hip) -- shared with the batched front end (batch.hip, batch_dev.h).
#pragma once
#include "grid.h"

struct ghicp_cloud {
  ghicp_ctx* ctx = nullptr;
  ghicp_pair_config cfg;
  long long n = 0, m = 0, k = 0, cand = 0;
  float bbx = 0.f;
  int V = 1;
  DevBuf ds;    // m float4 (down-sampled points; empty for handles rebuilt from stored features)
  DevBuf kp;    // k int32: keypoint ids into ds
  DevBuf kpx;   // k x 3 f64
  DevBuf feat;  // BSC: 4 x k x 56 bytes (variants 0..V-1 filled) | FPFH: k x 33 f32 | None: empty
  // what the cloud needs to serve as the TARGET of the batched fine registration (ghicp_cloud_prepare_refine, refine.hip): the fine and
  // coarse 1-NN grids over ds, and the k-NN normals of ds for k = rf_k (0: none).  Invalid after every recompute.
  bool rf_ready = false;
  int rf_k = 0;
  GridDesc rf_fine, rf_coarse;
  DevBuf rf_fpts, rf_fstart, rf_cpts, rf_cstart, rf_nrm;
  void rf_invalidate() { rf_ready = false; rf_k = 0; }
  void rf_release() { rf_invalidate(); rf_fpts.release(); rf_fstart.release(); rf_cpts.release(); rf_cstart.release(); rf_nrm.release(); }
  // what it needs for the batched generalized ICP (ghicp_cloud_prepare_gicp, refine_gicp.hip), as source or target: the m x 6 f64
  // regularised covariances of ds for (gc_k, gc_eps).  Invalid after every recompute; ghicp_cloud_prepare_refine keeps them.
  bool gc_ready = false;
  int gc_k = 0;
  double gc_eps = 0.0;
  DevBuf gc_cov;
  void gc_invalidate() { gc_ready = false; gc_k = 0; gc_eps = 0.0; }
  void gc_release() { gc_invalidate(); gc_cov.release(); }
  // what it needs to serve as the TARGET of the batched calOverlap (ghicp_cloud_prepare_overlap, overlap_clouds.hip): the search grid of
  // cell ov_thre over ds -- the grid ghicp_cal_overlap builds over its second cloud on every call.  Invalid after every recompute;
  // ghicp_cloud_prepare_refine and ghicp_cloud_prepare_gicp keep it.
  bool ov_ready = false;
  float ov_thre = 0.f;
  GridDesc ov_grid;
  DevBuf ov_pts, ov_start;  // m float4 in cell order; ncell + 1 cell starts
  void ov_invalidate() { ov_ready = false; ov_thre = 0.f; }
  void ov_release() { ov_invalidate(); ov_pts.release(); ov_start.release(); }
};

// the fine + coarse 1-NN grids over c->ds into the handle's own buffers (refine.hip); the caller sets rf_ready once the stream is idle
int gh_cloud_build_grids(ghicp_ctx* ctx, ghicp_cloud* c);

inline bool same_front_end(const ghicp_pair_config& a, const ghicp_pair_config& b) {
  return a.reg.feature == b.reg.feature && a.reg.dof == b.reg.dof && a.reg.radius_nonmax == b.reg.radius_nonmax && a.voxel == b.voxel &&
         a.neighborhood_radius == b.neighborhood_radius && a.ratio_max == b.ratio_max && a.min_neighbors == b.min_neighbors &&
         (a.reg.feature != GHICP_FEATURE_BSC || memcmp(a.pattern, b.pattern, sizeof(a.pattern)) == 0);
}
