// Internal: the front end's device-pointer entry points, declared ONCE -- included by every file that calls one (pair.hip, cloud.hip, batch.hip,
// filter.hip) and by every file that defines one.  C linkage: a definition whose parameter list drifts from the declaration here conflicts with
// it and does not compile (with C++ linkage it would be a silent overload that fails when the library is loaded).
#pragma once
#include "grid.h"

extern "C" {
int gh_voxel_filter_dev(ghicp_ctx* ctx, const float* xyz, long long n, int stride, float voxel, int32_t* keep, long long* m_out);  // grid.hip
int gh_keypoints_dev(ghicp_ctx* ctx, const float* xyz, long long m, int stride, float radius, float ratio_max, int min_n, float nms_radius,
                     int32_t* kp, long long* k_out);  // nms.hip
int gh_bsc_dev(ghicp_ctx* ctx, const float* xyz, long long m, int stride, const int32_t* kp, long long K, float R, int dof, const int32_t* pattern_host,
               uint8_t* feat, float* lcs);  // bsc.hip
int gh_fpfh_dev(ghicp_ctx* ctx, const float* xyz, long long m, int stride, float* normals_opt, float* hist);  // fpfh.hip
int gh_gather_rows33_dev(ghicp_ctx* ctx, const float* hist, const int32_t* idx, long long k, float* out);    // fpfh.hip
float gh_fpfh_cell(const float* mm, long long m);  // fpfh.hip: the cell size of the k-NN grid of one cloud
int gh_fpfh_batch_dev(ghicp_ctx* ctx, const float4* dsg, int M, const float4* pts, const unsigned* start, const GridDesc* gd_dev, const unsigned* cell_base_dev,
                      const int* moff_dev, int nb, float* hist);  // fpfh.hip
int gh_knn_prepare_batch_dev(ghicp_ctx* ctx, const float4* dsg, int M, const float4* pts, const unsigned* start, const GridDesc* gd_dev,
                             const unsigned* cell_base_dev, const int* moff_dev, int nb, int k, float* normals, double eps, double* cov6);  // fpfh.hip
int gh_fd_fpfh_dev(ghicp_ctx* ctx, const float* histS, int ks, const float* histT, int kt, float* FD);  // fd.hip
int gh_register_pairs_batched(ghicp_ctx* ctx, const ghicp_pair_config* cfg, int32_t n_pairs, const float* const* xyzS, const int64_t* nS,
                              const float* const* xyzT, const int64_t* nT, int stride, ghicp_pair_stats* stats, int* handled);  // cloud.hip
}
