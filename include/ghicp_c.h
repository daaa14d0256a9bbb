/* =====================================================================================
 *  ghicp_c.h -- C ABI of libghicp_hip.so: the MI355X (gfx950) GH-ICP registration hot path.
 *
 *  This is the drop-in boundary.  The reference has no FFI; its boundary is the
 *  public C++ class API.  Each entry point below names the reference method(s) it replaces
 *  (paths under the reference checkout).  The C++ headers next to this file (ghicp_reg.h, km.h,
 *  keypoint_detect.hpp, binary_feature_extraction.hpp, common_reg.h ...) keep the reference's
 *  class / method names and forward here.
 *
 *  Conventions
 *    - every function returns GHICP_OK (0) or an error code; ghicp_last_error() has the text.
 *    - bulk array arguments are DEVICE pointers by default.  After
 *      ghicp_ctx_set_host_pointers(ctx, 1) they are HOST pointers and the library stages them
 *      (this is what the C++ drop-in classes use).  Scalars / small outputs marked [host] are
 *      always host memory.
 *    - all work is enqueued on the context's stream (ghicp_ctx_set_stream); functions that
 *      return counts synchronise that stream.
 *    - point clouds are `float` with a stride in floats (3 = packed xyz, 4 = float4,
 *      8 = pcl::PointXYZI's 32-byte layout).
 *    - no cwd side effects, no stdout, re-entrant per context (unlike km.cpp:147 / bfe:96).
 * ===================================================================================== */
#ifndef GHICP_C_H_
#define GHICP_C_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ghicp_ctx ghicp_ctx;

enum {
  GHICP_OK = 0,
  GHICP_ERR_ARG = 1,      /* bad argument */
  GHICP_ERR_HIP = 2,      /* a HIP runtime call failed */
  GHICP_ERR_NO_GPU = 3,   /* no usable gfx950 device: the library has NO CPU fallback */
  GHICP_ERR_CAPACITY = 4, /* an output buffer / internal limit is too small */
  GHICP_ERR_INTERNAL = 5
};

/* include/utility.h:51-57 and :59-64 (same numeric values as the reference enums) */
enum { GHICP_FEATURE_BSC = 0, GHICP_FEATURE_ROPS = 1, GHICP_FEATURE_FPFH = 2, GHICP_FEATURE_NONE = 3 };
enum { GHICP_CORR_NN = 0, GHICP_CORR_NNR = 1, GHICP_CORR_KM = 2 };

/* GHRegistration ctor arguments (include/ghicp_reg.h:77-117) + Energyfunction::init constants
 * (include/ghicp_reg.h:26-41).  ghicp_params_default() fills the reference defaults. */
typedef struct ghicp_params {
  int32_t feature;  /* GHICP_FEATURE_* */
  int32_t corr;     /* GHICP_CORR_*    */
  int32_t dof;      /* 4 or 6 (only selects the number of source BSC variants, ghicp_reg.cpp:178-182) */
  int32_t max_iter; /* guard; the reference loops `while(!converge)` with none (ghicp_reg.cpp:49) */
  float radius_nonmax, adjust_ratio, adjust_step, est_iou;
  float converge_t, converge_r; /* 0.02 m / 0.02 deg (ghicp_reg.h:80) */
  float bbx_magnitude;          /* test/ghicp_main.cpp:91-93 */
  float pad_;
  double penalty_initial, para1, para2, km_eps;
  int32_t min_cor, weight_changing_rate;
} ghicp_params;

/* One iteration of GHRegistration::ghicp_reg (src/ghicp_reg.cpp:49-103): what the reference
 * prints / keeps in `energy, rmse, rmseafter, cor` (include/ghicp_reg.h:147-148). */
typedef struct ghicp_iter {
  int32_t cor, converged;
  double penalty, cdmean, cdstd, rmse, rmse_after, fdm, fdstd, iou, para1, para2, energy;
  double Rt[16]; /* Rt_temp of this iteration, row-major */
} ghicp_iter;

/* ------------------------------------------------------------------ context */
int ghicp_ctx_create(int device, ghicp_ctx** ctx);
int ghicp_ctx_destroy(ghicp_ctx* ctx);
/* The stream every call on this context is issued on.  The persistent pair loop of the Kuhn-Munkres batches forks onto auxiliary streams
 * of its own (one per LDS class of a batch) and joins them back into this stream; those streams follow ghicp_ctx_set_cu_mask, NOT a
 * compute-unit mask the caller may have put on a stream handed in here (the mask of a foreign stream is not inspected). */
int ghicp_ctx_set_stream(ghicp_ctx* ctx, void* hip_stream);
/* Gives the context its own stream restricted to the compute units whose bit is set (32 CUs per word); replaces any stream
 * set before.  Lets a pipeline keep some CUs free of the LDS-filling solve waves for another context's small kernels. */
int ghicp_ctx_set_cu_mask(ghicp_ctx* ctx, const uint32_t* mask, int32_t n_words);
int ghicp_ctx_set_host_pointers(ghicp_ctx* ctx, int on);
/* Host-pointer mode keeps the staged device copy of every LARGE POINT-CLOUD input (xyz rows, >= 256 KB; no other kind of argument)
 * between calls, keyed on host address, size and a fingerprint of the content, so that the reference's call sequence on one cloud -- CFilter::voxelfilter, CKeypointDetect, BSCEncoder /
 * FPFHfeature, transformPointCloud (test/ghicp_main.cpp:86-153) -- uploads it once (at most 1 GiB / 16 arrays, least recently used out
 * first).  Counters since the context was created: inputs served from a kept copy, inputs uploaded, bytes currently kept.  [host] outputs,
 * any may be NULL. */
int ghicp_ctx_stage_stats(const ghicp_ctx* ctx, int64_t* hits, int64_t* misses, int64_t* bytes_kept);
/* Frees every kept copy now (ghicp_ctx_set_host_pointers(ctx, 0) and ghicp_ctx_destroy do the same). */
int ghicp_ctx_stage_clear(ghicp_ctx* ctx);
int ghicp_ctx_synchronize(ghicp_ctx* ctx);
const char* ghicp_last_error(const ghicp_ctx* ctx);
/* Optional per-kernel timing (hipEvent brackets on the context's stream around the named kernels:
 * "pca_cells", "bsc", "km_solve", "cd_rowmin", "km_weights", "fd_bsc", "nms_round", "voxel_sort").
 * ghicp_ctx_kernel_time synchronises the stream; returns total ms and launch count since enabling. */
int ghicp_ctx_kernel_timing(ghicp_ctx* ctx, int on);
int ghicp_ctx_kernel_time(ghicp_ctx* ctx, const char* name, double* total_ms, int64_t* launches);
/* Launch records of the Kuhn-Munkres solve kernel collected while kernel timing is on: out8 = { launches, solves, mean solve ms,
 * mean over launches of the longest solve (ms), mean launch span (ms), solve slots resident on the chip, idle-slot fraction,
 * worst longest/mean ratio of a launch }.  (Diagnostics for the batched loop; the reference has no counterpart.) */
int ghicp_ctx_km_launch_stats(ghicp_ctx* ctx, double* out8);
/* Records of the persistent pair loop (Kuhn-Munkres configurations of ghicp_register_pairs / ghicp_register_clouds: one workgroup =
 * one solve slot runs a pair's whole ghicp_reg loop, src/ghicp_reg.cpp:49-103, and then pops the next pair), collected while kernel
 * timing is on: out12 = { batches, workgroups that ran, solves, mean solve ms, longest solve ms, mean batch span ms, idle-slot fraction
 * (1 - slot lifetimes / (resident slots x span): the tail of a batch), share of the slot lifetimes spent inside Kuhn-Munkres solves,
 * mean ms per pair-iteration in the statistics sweep, in the graph build, in the tail after the solve, 0 }.  (TWELVE doubles: the stage
 * times were appended to the eight of earlier versions.) */
int ghicp_ctx_pair_loop_stats(ghicp_ctx* ctx, double* out12);
/* Diagnostics: Kuhn-Munkres solves of this context's batched loops (ghicp_register_pairs / ghicp_register_clouds, Ct = KM) that went through the
 * solver's literal single-lane fallback since the context was created (rule R4's hazard check, km4_dev.h: correct, slow by design;
 * expected 0 on finite inputs -- a non-zero count explains multi-second solves). */
int ghicp_ctx_loop_hazards(ghicp_ctx* ctx, int64_t* solves /*[host]*/);
/* Scheduling hint for the NEXT batched Kuhn-Munkres registration on this context (ghicp_register_clouds / ghicp_register_pairs with
 * exactly n_pairs pairs; consumed by that call, ignored otherwise): cost[i] = expected relative TIME of pair i in a solve slot, e.g.
 * iterations x keypoints of the same pair last time, or any prior.  The solve slots of the persistent pair loop take the costliest pairs
 * of each class first (graphs that fit four slots per CU form ONE class, i.e. one queue: longest processing time first over the batch),
 * so that the slowest registrations (112 iterations against a mean of 35 on the TLS bench scenes) do not start in the middle of a batch
 * and leave the chip to a handful of stragglers; the share of the CUs the three-slots-per-CU class is confined to follows the hints'
 * sums.  Results do not depend on the hints (pairs share nothing); [host] array. */
int ghicp_ctx_set_loop_cost_hints(ghicp_ctx* ctx, int32_t n_pairs, const float* cost);
/* Diagnostics: the slot timeline of the LAST persistent batch that ran on this context while kernel timing was on -- per pair of the
 * batch (in the order of the call) three int64: when a solve slot took the pair, when it let go (device real-time clock, 100 MHz ticks,
 * bits [51:0]), and the pair's iterations (bits [15:0]).  The spare bits carry what the stragglers of a batch are looked up by:
 * out3[0] [55:52] compute unit, [56] shader array, [59:57] shader engine, [63:60] die (XCC) the slot ran on; out3[2] [31:16] the iteration of
 * the pair's longest Kuhn-Munkres solve, [63:32] that solve's duration in units of 160 ns.
 * out3 may be NULL (only *n_pairs is written); at most cap_pairs triples are copied. */
int ghicp_ctx_loop_timeline(ghicp_ctx* ctx, int64_t* out3, int64_t cap_pairs, int64_t* n_pairs);
/* Progress of the batched loop (ghicp_register_pairs / ghicp_register_clouds) currently running on this context: pairs that are still
 * iterating and pairs of the batch.  No device work; may be called from another thread while the loop runs (a scheduler can start the
 * next batch's front ends when only the slowly converging pairs are left). */
int ghicp_ctx_loop_progress(const ghicp_ctx* ctx, int64_t* active, int64_t* total);
/* Declares a batch of `total` pairs as about to start on this context (active = total) -- for a scheduler that publishes "the batch has
 * started" to other threads BEFORE it calls ghicp_register_clouds, so that they never read the previous batch's finished state. */
int ghicp_ctx_loop_progress_reset(ghicp_ctx* ctx, int64_t total);
const char* ghicp_version(void);
void ghicp_params_default(ghicp_params* p);

/* ------------------------------------------------------------------ front end (per cloud) */
/* CFilter::voxelfilter (include/filter.hpp:28-88, incl. its phantom-entry quirk: output row 0 is
 * a copy of input point 0).  keep_idx: capacity n+1 int32; *m [host]. */
int ghicp_voxel_filter(ghicp_ctx* ctx, const float* xyz, int64_t n, int stride, float voxel, int32_t* keep_idx, int64_t* m);
/* CFilter::SORFilter (include/filter.hpp:90-102) = pcl::StatisticalOutlierRemoval::applyFilterIndices as recalled (PCL 1.7 / 1.8; not
 * checked against its sources -- this comment and DESIGN.md N9 are the one place to correct it).  mean_k in 1..63 (the query and its
 * neighbours fill the 64 lanes of one wavefront); anything else is GHICP_ERR_ARG.  Finite coordinates are a precondition.
 *   per point    the mean_k + 1 nearest neighbours in the same cloud, query included; float squared L2 (d2 = dx*dx; d2 += dy*dy;
 *                d2 += dz*dz, no contraction); the list sorted by d2, entry 0 dropped, sqrtf(d2[t]) summed for t = 1 .. mean_k in
 *                ascending order in f64, divided by mean_k, rounded to float.  Only the multiset of the mean_k + 1 smallest d2 matters.
 *   statistics   sum and sq_sum of the float distances in f64 -- tiles of 1024 consecutive indices added in index order, then the tiles
 *                in index order (N9) --, mean = sum / n, variance = (sq_sum - sum*sum/n) / (n - 1), threshold = mean + std_mul * sqrt(variance)
 *   kept         point i stays iff !(dist[i] > threshold), the float promoted to f64; input order is kept
 *   n < mean_k + 1   PCL gets short result lists: every distance is 0, no point is valid, the threshold is NaN and every point stays
 *                (m = n, stats4 = NaN, NaN, NaN, 0)
 * ghicp_knn_mean_distance is the per-point stage alone: dist, n floats. */
int ghicp_knn_mean_distance(ghicp_ctx* ctx, const float* xyz, int64_t n, int stride, int mean_k, float* dist);
/* keep_idx: capacity n int32, the kept points' indices, ascending; *m [host]; stats4 [host] (may be NULL) = mean, stddev, threshold, valid count. */
int ghicp_sor_filter(ghicp_ctx* ctx, const float* xyz, int64_t n, int stride, int mean_k, double std_mul, int32_t* keep_idx, int64_t* m,
                     double* stats4);
/* CFilter::DisFilter (include/filter.hpp:105-117) as written (quirk Q10): point i stays iff (double)(float)(x*x + y + y) < xy_dis_max^2 &&
 * z < z_max && z > z_min -- `+ y + y`, not `+ y*y`.  keep_idx: capacity n, ascending; *m [host]. */
int ghicp_dis_filter(ghicp_ctx* ctx, const float* xyz, int64_t n, int stride, double xy_dis_max, double z_min, double z_max, int32_t* keep_idx,
                     int64_t* m);
/* CFilter::ActiveObjectFilter (include/filter.hpp:119-140): a point STRICTLY inside any box leaves (float coordinates against the f64
 * bounds; a point on a face stays, Q11).  boxes6 [host] = n_boxes x (min_x, min_y, min_z, max_x, max_y, max_z); n_boxes = 0 keeps every point. */
int ghicp_box_filter(ghicp_ctx* ctx, const float* xyz, int64_t n, int stride, const double* boxes6, int32_t n_boxes, int32_t* keep_idx,
                     int64_t* m);
/* The stable sort behind the voxel filter, the grids and the NMS order (the reference's std::sort calls, include/filter.hpp:66 and
 * include/keypoint_detect.hpp:119-130, made deterministic: equal keys keep their input order).  Ascending on the key bits
 * [bit_begin, bit_end) of n keys of key_bytes (4 or 8) bytes each; vals_in / vals_out (u32) may both be NULL (keys only).  The inputs are
 * left untouched.  Out of place: the four arrays (n items each) must not share a byte -- vals_out == vals_in, an output that overlaps
 * an input or the other output, even by a partial range, is GHICP_ERR_ARG and nothing is written. */
int ghicp_sort_pairs(ghicp_ctx* ctx, int key_bytes, const void* keys_in, void* keys_out, const uint32_t* vals_in, uint32_t* vals_out, int64_t n,
                     int bit_begin, int bit_end);
/* The same sort, segment by segment in one call (the clouds of a batched front end): segment s is the items [seg_off[s], seg_off[s + 1]) of
 * the arrays, seg_off [host] = n_segs + 1 ascending offsets from 0, 1 <= n_segs <= 64, empty segments allowed; each segment is sorted, stably,
 * on the bits [bit_begin, bit_begin + bits) of key - seg_base[s].  seg_base (4-byte keys only; n_segs words, like the arrays a device pointer
 * unless the context stages host pointers) may be NULL for 0; every key of a segment must be >= its base.  max_digit_bits: 8 or 9, the widest
 * digit of a place (0: the context's default); the digit places are planned from `bits`.  Buffers as for ghicp_sort_pairs. */
int ghicp_sort_segments(ghicp_ctx* ctx, int key_bytes, const void* keys_in, void* keys_out, const uint32_t* vals_in, uint32_t* vals_out, int32_t n_segs,
                        const int64_t* seg_off, const uint32_t* seg_base, int bit_begin, int bits, int max_digit_bits);
/* Test hook of the batched front end's sorts: the kernels that make the voxel and cell keys leave the first digit place's per-tile counts
 * for the sort.  With the check on, every such sort takes the counts again from the keys and compares (GHICP_ERR_INTERNAL when they differ; a
 * host round trip per sort).  *checked / *mismatched: sorts compared / found different since the context was created. */
int ghicp_ctx_set_sort_hist_check(ghicp_ctx* ctx, int on);
int ghicp_ctx_sort_hist_checks(ghicp_ctx* ctx, int64_t* checked, int64_t* mismatched);
/* The other device-wide primitives under the front end (prims.hip), as primitives; n < 2^31 - 2 as for the sort, n == 0 is fine.
 * Inclusive prefix sum in place, modulo 2^32: data[i] = data[0] + ... + data[i].  `data` needs the alignment of its type only. */
int ghicp_scan_inclusive_u32(ghicp_ctx* ctx, uint32_t* data, int64_t n);
/* out[0 .. *count) = vals[i] -- or the position i itself when vals is NULL -- of every i with flags[i] != 0 (any non-zero byte), in
 * ascending order of i.  out: capacity n, only the first *count items are written; it may not overlap flags or vals.  *count [host]. */
int ghicp_select_flagged(ghicp_ctx* ctx, const uint8_t* flags, const uint32_t* vals, int64_t n, uint32_t* out, int64_t* count);
/* out[0 .. *count) = the distinct values of the ASCENDING array keys (the head of every run of equal keys), ascending.  out: capacity n,
 * only the first *count items are written; it may not overlap keys.  *count [host]. */
int ghicp_unique_sorted_u32(ghicp_ctx* ctx, const uint32_t* keys, int64_t n, uint32_t* out, int64_t* count);
/* gather rows: out[i] = xyz[idx[i]] as packed float4 (x,y,z,0). */
int ghicp_gather_points(ghicp_ctx* ctx, const float* xyz, int stride, const int32_t* idx, int64_t m, float* out_xyz4);
/* bbx_magnitude of test/ghicp_main.cpp:91-93 (CloudUtility::getCloudBound, utility.h:153-183). [host] out */
int ghicp_bbx_magnitude(ghicp_ctx* ctx, const float* xyz, int64_t n, int stride, float* bbx);
/* CloudUtility::getCloudBound (include/utility.h:153-183): min_x, min_y, min_z, max_x, max_y, max_z as doubles holding the float
 * extremes. [host] out6; n == 0 is an argument error (the reference reads cloud[0]). */
int ghicp_cloud_bounds(ghicp_ctx* ctx, const float* xyz, int64_t n, int stride, double* out6);

/* PrincipleComponentAnalysis::CalculatePcaFeaturesOfPointCloud(cloud, features, float radius)
 * (include/pca.h:133-165, 202-250).  lambda: m x 3 f32 (descending), curvature: m f64, count: m i32. */
int ghicp_pca_curvature(ghicp_ctx* ctx, const float* xyz, int64_t m, int stride, float radius, float* lambda, double* curvature,
                        int32_t* count);
/* CKeypointDetect::pruneUnstablePoints (include/keypoint_detect.hpp:132-147). cand: capacity m; *c [host]. */
int ghicp_prune(ghicp_ctx* ctx, const float* lambda, const int32_t* count, int64_t m, float ratio_max, int min_n, int32_t* cand,
                int64_t* c);
/* CKeypointDetect::nonMaximaSuppression (include/keypoint_detect.hpp:149-191).  kp: capacity c,
 * output in descending-curvature order; *k [host]. */
int ghicp_nms(ghicp_ctx* ctx, const float* xyz, int stride, const double* curvature, const int32_t* cand, int64_t c, float radius,
              int32_t* kp, int64_t* k);
/* CKeypointDetect::keypointDetectionBasedOnCurvature (include/keypoint_detect.hpp:27-51):
 * PCA -> prune -> NMS.  kp_idx: capacity m; *k [host]. */
int ghicp_keypoints(ghicp_ctx* ctx, const float* xyz, int64_t m, int stride, float radius, float ratio_max, int min_n, float nms_radius,
                    int32_t* kp_idx, int64_t* k);
/* CKeypointDetect::keypointDetectionBasedOnCurvature_adaptive (include/keypoint_detect.hpp:53-111).  The reference's
 * constants are upper = 50000, lower = 5000; ratio_used / rounds [host] (may be NULL) report the final threshold and the
 * number of extra prune + NMS rounds. */
int ghicp_keypoints_adaptive(ghicp_ctx* ctx, const float* xyz, int64_t m, int stride, float radius, float ratio_max, int min_n,
                             float nms_radius, int64_t upper, int64_t lower, int32_t* kp_idx, int64_t* k, float* ratio_used,
                             int32_t* rounds);

/* BSCEncoder::extractBinaryFeatures (include/binary_feature_extraction.hpp:603-676).
 * pattern: 49 x 2 int32 [host] (the sample_pattern.txt content, bfe:63-117).
 * feat: 4 x k x 56 bytes (variants beyond the dof's count are zero), lcs: k x 12 f32 (x,y,z axes, origin). */
int ghicp_bsc_encode(ghicp_ctx* ctx, const float* xyz, int64_t m, int stride, const int32_t* kp_idx, int64_t k, float radius, int dof,
                     const int32_t* pattern, uint8_t* feat, float* lcs);

/* FPFHfeature::compute_fpfh_feature (include/fpfh.hpp:36-58): pcl::NormalEstimation k=20 + pcl::FPFHEstimationOMP k=20
 * over the whole cloud.  normals: m x 3 f32 or NULL; hist: m x 33 f32 (pcl::FPFHSignature33 rows). */
int ghicp_fpfh(ghicp_ctx* ctx, const float* xyz, int64_t m, int stride, int k_normal, int k_feature, float* normals, float* hist);
/* FPFHfeature::keyfpfh (include/fpfh.hpp:93-115): out[i] = hist[kp_idx[i]] (k x 33). Device pointers. */
int ghicp_fpfh_keypoints(ghicp_ctx* ctx, const float* hist, const int32_t* kp_idx, int64_t k, float* out);

/* ------------------------------------------------------------------ per pair */
/* GHRegistration::calFD_BSC (src/ghicp_reg.cpp:143-200) + StereoBinaryFeature::hammingDistance
 * (src/stereo_binary_feature.cpp:87-104).  featS: V x ks x 56, featT: kt x 56, FD: ks x kt u16 row-major. */
int ghicp_fd_bsc(ghicp_ctx* ctx, const uint8_t* featS, int64_t ks, int V, const uint8_t* featT, int64_t kt, uint16_t* FD);
/* GHRegistration::calFD_FPFH (src/ghicp_reg.cpp:202-214) + FPFHfeature::compute_fpfh_distance
 * (include/fpfh.hpp:135-165).  hist: k x 33 f32, FD: ks x kt f32 row-major. */
int ghicp_fd_fpfh(ghicp_ctx* ctx, const float* histS, int64_t ks, const float* histT, int64_t kt, float* FD);

/* Km::kmsolve (src/km.cpp:40-126): w is n x n f64 row-major, match[y] = x (int32, n). */
int ghicp_km_solve(ghicp_ctx* ctx, const double* w, int64_t n, double eps, int32_t* match);

/* pcl::registration::TransformationEstimationSVD as used by GHRegistration::transformestimation
 * (src/ghicp_reg.cpp:839-866): c x 3 f64 correspondences (cast to f32 like the reference), Rt 4x4 [host]. */
int ghicp_rigid_svd(ghicp_ctx* ctx, const double* src, const double* tgt, int64_t c, double* Rt16);
/* The same solve on the host (same numerics contract, no context, no GPU): for the few-point closed-form solvers of the
 * reference's API (CRegistration::SVD_6DOF, src/common_reg.cpp:774-888).  src/tgt: c x 3 f64 host arrays. */
int ghicp_rigid_svd_host(const double* src, const double* tgt, int64_t c, double* Rt16);

/* GHRegistration::ghicp_reg (src/ghicp_reg.cpp:24-112): the whole iteration loop
 * (calED, calCD_*, findcorrespondence{NN,NNR,KM}, transformestimation, adjustweight).
 *   kpS: ks x 3 f64, kpT: kt x 3 f64 (Keypoints::setCoordinate, ghicp_reg.h:53-59); kpS is not modified.
 *   FD : ks x kt row-major; u16 for BSC, f32 for FPFH, NULL for None.
 *   Rt16 [host] final 4x4 (Source -> Target); trace [host] capacity max_iter or NULL;
 *   n_iter [host]; matchlist: max_iter x ks int32 (T index or -1) or NULL. */
int ghicp_register(ghicp_ctx* ctx, const ghicp_params* p, const double* kpS, int64_t ks, const double* kpT, int64_t kt, const void* FD,
                   double* Rt16, ghicp_iter* trace, int32_t* n_iter, int32_t* matchlist);

/* One iteration at a time: the body of the while loop of GHRegistration::ghicp_reg (src/ghicp_reg.cpp:49-103) -- calED, calCD_*, the
 * correspondence search, transformestimation (which moves the source keypoints and accumulates Rt_tillnow), adjustweight -- as one call.
 * ghicp_loop_create copies the inputs (same meaning as ghicp_register's) into a state object; every ghicp_iterate runs exactly one
 * iteration on it and returns that iteration's record (`out`, [host]; out->converged is the loop's exit test, ghicp_reg.cpp:796-803,
 * 909-914) and, when match_row is not NULL, its correspondences (ks int32: T index or -1).  A sequence of ghicp_iterate calls until
 * out->converged reproduces ghicp_register's trace bit for bit; calling it again after convergence is an argument error.
 * ghicp_loop_result: the accumulated 4x4 (Rt_tillnow), iterations done, the converged flag, RMSE-after of the last iteration. */
typedef struct ghicp_loop ghicp_loop;
int ghicp_loop_create(ghicp_ctx* ctx, const ghicp_params* p, const double* kpS, int64_t ks, const double* kpT, int64_t kt, const void* FD,
                      ghicp_loop** out);
int ghicp_iterate(ghicp_ctx* ctx, ghicp_loop* loop, ghicp_iter* out, int32_t* match_row);
int ghicp_loop_result(const ghicp_loop* loop, double* Rt16, int32_t* n_iter, int32_t* converged, double* rmse_after);
void ghicp_loop_destroy(ghicp_loop* loop);

/* pcl::transformPointCloud(cloud, out, Rt.cast<float>()) (test/ghicp_main.cpp:153). out: n x 3 packed f32. */
int ghicp_transform_cloud(ghicp_ctx* ctx, const float* xyz, int64_t n, int stride, const double* Rt16_host, float* out_xyz);
/* The same for the raw sources of a whole batch of registered pairs in one launch: cloud i (xyz[i], n[i] rows of `stride` floats) under
 * Rt16_host[16 i .. 16 i + 15] into out[i] (n[i] x 3 packed f32).  [host] pointer tables and matrices, device clouds; bit-identical to
 * ghicp_transform_cloud cloud by cloud.  Device-pointer mode only. */
int ghicp_transform_clouds(ghicp_ctx* ctx, int32_t n_clouds, const float* const* xyz, const int64_t* n, int stride, const double* Rt16_host,
                           float* const* out_xyz);

/* ------------------------------------------------------------------ whole pair (test/ghicp_main.cpp:86-153) */
typedef struct ghicp_pair_config {
  ghicp_params reg;         /* bbx_magnitude is computed from the down-sampled source and overwritten */
  float voxel;              /* argv[6]; <= 0 skips the voxel filter */
  float neighborhood_radius;/* argv[7] */
  float ratio_max;          /* 0.65 (main:96) */
  int32_t min_neighbors;    /* 20   (main:97) */
  int32_t pattern[98];      /* BSC sample pattern */
} ghicp_pair_config;

typedef struct ghicp_pair_stats {
  int64_t n_s, n_t, m_s, m_t, k_s, k_t; /* raw, down-sampled, keypoints */
  int32_t iterations, converged;
  double Rt[16];
  float bbx_magnitude;
  float ms_voxel, ms_keypoints, ms_feature, ms_fd, ms_loop, ms_total; /* hipEvent timings */
  float pad_;
  /* src/ghicp_reg.cpp:918-924: at convergence the reference prints "Registration Succeed." iff RMSEafter < 1.5 * nonmax
   * (RMSE of the last iteration's correspondences after its transform), else "Registration Failed.".  registered_ok is that
   * verdict (0 when the loop stopped at the max_iter guard); rmse_after is the value it was taken from. */
  double rmse_after;
  int32_t registered_ok, pad2_;
} ghicp_pair_stats;

/* voxel -> keypoints -> feature -> FD -> loop for one (S,T); raw clouds are device (or host) xyz. */
int ghicp_register_pair(ghicp_ctx* ctx, const ghicp_pair_config* cfg, const float* xyzS, int64_t nS, const float* xyzT, int64_t nT,
                        int stride, ghicp_pair_stats* stats /*[host]*/, ghicp_iter* trace /*[host] or NULL*/);

/* A batch of independent pairs (BASELINE configs[3]: many fragment pairs per GPU): the per-pair front ends run
 * back to back, then one batched GH-ICP loop advances every pair concurrently (one KM solve per wave).
 * Device pointers only.  xyzS/xyzT/nS/nT: host arrays of n_pairs device pointers / sizes; stats: n_pairs [host]. */
int ghicp_register_pairs(ghicp_ctx* ctx, const ghicp_pair_config* cfg, int32_t n_pairs, const float* const* xyzS, const int64_t* nS,
                         const float* const* xyzT, const int64_t* nT, int stride, ghicp_pair_stats* stats);


/* ------------------------------------------------------------------------------------------------
 * Fine registration: CRegistration<PointT> (include/common_reg.h:26-110, src/common_reg.cpp).
 * The reference wraps PCL's IterativeClosestPoint / IterativeClosestPointWithNormals; these entry
 * points run the same loop (1-NN correspondences, optional reciprocal test and trimmed rejector,
 * closed-form solve, PCL's default convergence criteria) on the device.
 * ------------------------------------------------------------------------------------------------ */
enum { GHICP_ICP_POINT_TO_POINT = 0, GHICP_ICP_POINT_TO_PLANE = 1 };
/* pcl::registration::DefaultConvergenceCriteria::ConvergenceState */
enum { GHICP_ICP_NOT_CONVERGED = 0, GHICP_ICP_ITERATIONS = 1, GHICP_ICP_TRANSFORM = 2, GHICP_ICP_ABS_MSE = 3, GHICP_ICP_REL_MSE = 4,
       GHICP_ICP_NO_CORRESPONDENCES = 5 };

typedef struct ghicp_icp_params {
  int32_t max_iter;        /* icp_reg / ptplicp_reg argument (common_reg.cpp:51,130) */
  int32_t use_reciprocal;  /* use_reciprocal_correspondence */
  int32_t use_trimmed;     /* use_trimmed_rejector: overlap = calOverlap(S, T, thre_dis) */
  int32_t metric;          /* GHICP_ICP_POINT_TO_POINT (icp_reg) or GHICP_ICP_POINT_TO_PLANE (ptplicp_reg) */
  float thre_dis;          /* search radius of the overlap estimate */
  float min_overlap;       /* min_overlap_for_reg: below it the registration is refused (reference returns false) */
  int32_t covariance_k;    /* ptplicp_reg: k of the target normals (CalculatePointCloudWithNormal_KNN), <= 20 */
  int32_t pad_;
  double transformation_epsilon;     /* 1e-8 (common_reg.cpp:82,156) */
  double euclidean_fitness_epsilon;  /* 1e-5 (common_reg.cpp:84,158) */
} ghicp_icp_params;

typedef struct ghicp_icp_stats {
  int32_t done;        /* 0: refused because overlap < min_overlap (T untouched), 1: ran */
  int32_t iterations;
  int32_t converged;
  int32_t reason;      /* GHICP_ICP_* convergence state */
  int64_t correspondences; /* used by the last solve */
  float overlap;       /* calOverlap result when use_trimmed, else 0 */
  float pad_;
  double mse;          /* mean squared correspondence distance of the last iteration */
  double fitness;      /* getFitnessScore(): mean squared 1-NN distance of the transformed source */
} ghicp_icp_stats;

void ghicp_icp_params_default(ghicp_icp_params* p);

/* CRegistration::calOverlap (common_reg.cpp:294-317): share of cloud1 points with a cloud2 point at d^2 < thre_dis^2,
 * (0.01 + count) / n1. */
int ghicp_cal_overlap(ghicp_ctx* ctx, const float* xyz1, int64_t n1, int stride1, const float* xyz2, int64_t n2, int stride2, float thre_dis,
                      float* ratio /*[host]*/);

/* CRegistration::icp_reg (common_reg.cpp:45-107) and ptplicp_reg (122-199), selected by params->metric.
 * T16: row-major float 4x4 source->target [host]; transformed: ns x 3 (device/host per mode) or NULL. */
int ghicp_icp(ghicp_ctx* ctx, const float* xyzS, int64_t ns, int strideS, const float* xyzT, int64_t nt, int strideT,
              const ghicp_icp_params* params, float* T16 /*[host]*/, float* transformed, ghicp_icp_stats* stats /*[host]*/);

/* PrincipleComponentAnalysis::CalculateNormalVector_KNN (include/pca.h:92-109): k-NN normals + CheckNormals. */
int ghicp_knn_normals(ghicp_ctx* ctx, const float* xyz, int64_t n, int stride, int k, float* normals /*n x 3*/);

/* exact 1-NN of every query in the target (the correspondence step of the ICP loop): ties -> lower target index. */
int ghicp_nn_search(ghicp_ctx* ctx, const float* query, int64_t nq, int strideQ, const float* xyzT, int64_t nt, int strideT,
                    int32_t* idx /*nq*/, float* d2 /*nq*/);

/* CRegistration::invTransform (common_reg.cpp:357-370): R^T with the NEGATED translation, as the reference does. */
void ghicp_inv_transform(const float* T16, float* inv16);

/* CRegistration::transformcloud (common_reg.cpp:325-349): float 4x4 * (x, y, z, 1). */
int ghicp_transform_cloud_f32(ghicp_ctx* ctx, const float* xyz, int64_t n, int stride, const float* T16 /*[host]*/, float* out /*n x 3*/);

/* CRegistration::gicp_reg (common_reg.cpp:216-284): pcl::GeneralizedIterativeClosestPoint configured by the reference.  PCL's GICP
 * as recalled (PCL 1.7 / 1.8; not checked against its sources -- this comment and DESIGN.md §4a are the one place to correct it):
 *   covariances  every point's k nearest neighbours in its own cloud (query included), mean + 1/k scatter, eigenvectors U,
 *                C = U diag(1, 1, gicp_epsilon) U^T (the smallest eigenvalue replaced by gicp_epsilon), f64
 *   outer loop   source points under transformation_ (float), 1-NN in the target, kept if d^2 < max_correspondence_distance^2;
 *                per correspondence M_i = (R C_S,i R^T + C_T,j)^-1 in f64 (R of transformation_)
 *   inner        minimise (1/c) sum r_i^T M_i r_i over x = (tx, ty, tz, roll, pitch, yaw), R(x) = Rz(yaw) Ry(pitch) Rx(roll),
 *                from the parameters of transformation_.  PCL uses BFGS; here the solver is the contract's own:
 *                Gauss-Newton with the analytic Jacobian, at most max_inner_iter steps, stop once max |dx| < 1e-10.
 *                Fewer than 4 correspondences: PCL throws and the loop stops unconverged (reason GHICP_ICP_NO_CORRESPONDENCES).
 *   convergence  delta = max over the 4x4 of |prev - cur|, the 3x3 block scaled by 1/rotation_epsilon, the rest by
 *                1/transformation_epsilon; converged when iterations >= max_iter (GHICP_ICP_ITERATIONS) or delta < 1
 *                (GHICP_ICP_TRANSFORM)
 *   output       final = transformation_, transformed = final * S, fitness = getFitnessScore()
 * GICP's computeTransformation does its own 1-NN search: the reference's reciprocal flag has no effect and its trimmed rejector is
 * never consulted (common_reg.cpp:213-215).  use_trimmed therefore acts only as the overlap gate (refusal below min_overlap); the calls that
 * do apply the rejector are separate entry points (ghicp_gicp_trimmed_from, ghicp_gicp_clouds_trimmed). */
typedef struct ghicp_gicp_params {
  int32_t max_iter;        /* gicp_reg argument */
  int32_t use_reciprocal;  /* accepted, no effect (see above) */
  int32_t use_trimmed;     /* overlap gate only: calOverlap(S, T, thre_dis) < min_overlap refuses */
  int32_t covariance_k;    /* setCorrespondenceRandomness: k of the covariances of both clouds, 1..20 */
  float thre_dis;
  float min_overlap;
  int32_t max_inner_iter;  /* Gauss-Newton steps per outer iteration, 1..100 (20) */
  int32_t pad_;
  double max_correspondence_distance; /* 1e6 (common_reg.cpp:253) */
  double gicp_epsilon;                /* 1e-3 */
  double transformation_epsilon;      /* 1e-8 (common_reg.cpp:263) */
  double rotation_epsilon;            /* 1e-6 (common_reg.cpp:265) */
} ghicp_gicp_params;

/* GHICP_ERR_ARG when p is NULL. */
int ghicp_gicp_params_default(ghicp_gicp_params* p);

/* CRegistration::gicp_reg.  Same conventions as ghicp_icp: T16 row-major float 4x4 [host], transformed ns x 3 or NULL; stats->mse is the
 * mean squared 1-NN distance of the last iteration's correspondences. */
int ghicp_gicp(ghicp_ctx* ctx, const float* xyzS, int64_t ns, int strideS, const float* xyzT, int64_t nt, int strideT,
               const ghicp_gicp_params* params, float* T16 /*[host]*/, float* transformed, ghicp_icp_stats* stats /*[host]*/);

/* ghicp_gicp from an initial pose: transformation_ starts at guess16 (row-major float 4x4 [host], source -> target; NULL: the identity,
 * which is ghicp_gicp itself, bit for bit).  The source points and the source covariances stay in the source's OWN frame: every outer
 * iteration moves the points by the current transformation_ for the 1-NN search and rotates C_S,i by its R (M_i above), so covariances
 * computed once per cloud serve every pair and every guess.  As recalled (same caveat as above), this is what PCL's own
 * align(output, guess) does.  The reference calls align without a guess (common_reg.cpp:216-284): the guess is an EXTENSION of this ABI,
 * the stage after a coarse GH-ICP pose.
 *   overlap gate  with use_trimmed: calOverlap of the guess-moved source (the float expression of ghicp_transform_cloud_f32) against T
 *   outputs       T16 = the final transformation_, the TOTAL source -> target pose (guess included); transformed = T16 * S.  Fewer than 4
 *                 correspondences: T16 = the guess.  A refused pair leaves T16 untouched.
 *   GHICP_ERR_ARG for a guess with a non-finite entry or a last row other than (0, 0, 0, 1); whether the 3x3 block is a rotation is the
 *                 caller's business, as everywhere in this ABI. */
int ghicp_gicp_from(ghicp_ctx* ctx, const float* xyzS, int64_t ns, int strideS, const float* xyzT, int64_t nt, int strideT,
                    const ghicp_gicp_params* params, const float* guess16 /*[host] row-major 4x4, NULL = identity*/,
                    float* T16 /*[host]*/, float* transformed, ghicp_icp_stats* stats /*[host]*/);

/* ghicp_gicp_from with the trimmed rejector APPLIED (opt-in; the reference's gicp_reg takes use_trimmed_rejector but PCL's GICP never
 * consults it, and ghicp_gicp / ghicp_gicp_from / ghicp_gicp_clouds keep that: there use_trimmed is the gate alone).  Every outer iteration:
 *   1. the source under transformation_;  2. its 1-NN in the target;
 *   3. correspondences with d^2 >= max_correspondence_distance^2 are rejected; the survivors are `count`;
 *   4. of those, the nv = min(count, floor(ratio * float(count))) smallest by the key (float d^2 bits, source index) are kept -- the rule and
 *      the tie-break of ghicp_icp's trimmed rejector (CorrespondenceRejectorTrimmed): ranked by Euclidean d^2, not by Mahalanobis distance;
 *   5. M_i, the count and the MSE over the kept set only;
 *   6. nv < 4: GHICP_ICP_NO_CORRESPONDENCES, as ghicp_gicp_from for count < 4 (T16 = the guess when it happens in the first iteration).
 * ratio is fixed for the whole registration, as in icp_reg: trim_ratio in (0, 1] is used as given; trim_ratio == 0 means the calOverlap
 * estimate of the gate (this is how icp_reg feeds its rejector) and requires params->use_trimmed = 1.  stats->correspondences and stats->mse
 * describe the kept set of the last iteration.  The inner solver, the convergence test, the fitness, the guess and the gate are those of
 * ghicp_gicp_from; trim_ratio == 1 is ghicp_gicp_from itself, bit for bit.
 * GHICP_ERR_ARG as ghicp_gicp_from, and for a trim_ratio that is negative, above 1 or not finite, or 0 without use_trimmed. */
int ghicp_gicp_trimmed_from(ghicp_ctx* ctx, const float* xyzS, int64_t ns, int strideS, const float* xyzT, int64_t nt, int strideT,
                            const ghicp_gicp_params* params, const float* guess16 /*[host] row-major 4x4, NULL = identity*/, float trim_ratio,
                            float* T16 /*[host]*/, float* transformed, ghicp_icp_stats* stats /*[host]*/);

/* The regularised covariances of one cloud as ghicp_gicp computes them: n x 6 f64 (c00, c01, c02, c11, c12, c22). k in 1..20. */
int ghicp_gicp_covariances(ghicp_ctx* ctx, const float* xyz, int64_t n, int stride, int k, double eps, double* cov6);

/* ------------------------------------------------------------------------------------------------
 * Per-cloud front-end cache (multi-view / all-pairs registration): down-sampling, keypoints and
 * descriptors of one cloud (test/ghicp_main.cpp:86-127) computed once and kept in HBM; a pair then costs
 * only calFD_* and the loop.  Results are identical to ghicp_register_pairs on the same clouds.
 * ------------------------------------------------------------------------------------------------ */
typedef struct ghicp_cloud ghicp_cloud;

typedef struct ghicp_cloud_info {
  int64_t n, m, k;        /* raw points, down-sampled points, keypoints */
  int32_t variants;       /* V: BSC strings per keypoint (1, 2 or 4; binary_feature_extraction.hpp:648-660) */
  int32_t feature;        /* GHICP_FEATURE_* */
  float bbx_magnitude;    /* of the down-sampled cloud (main:91-93) */
  int32_t candidates;     /* points that passed pruneUnstablePoints (keypoint_detect.hpp:132-147) = input of the NMS; 0 when not recorded */
  int64_t feature_bytes;  /* BSC: V*k*56, FPFH: k*33*4, None: 0 */
} ghicp_cloud_info;

int ghicp_cloud_create(ghicp_ctx* ctx, const ghicp_pair_config* cfg, const float* xyz, int64_t n, int stride, ghicp_cloud** out);
/* rebuilds a handle from stored results: kp_xyz k x 3 f64, feat = V*k*56 BSC bytes (variant-major) or k x 33 f32 FPFH rows */
int ghicp_cloud_from_features(ghicp_ctx* ctx, const ghicp_pair_config* cfg, const double* kp_xyz, int64_t k, const void* feat,
                              float bbx_magnitude, ghicp_cloud** out);
/* recomputes a handle for another raw cloud with the configuration it was created with, reusing its buffers (no
 * allocation in a steady-state pipeline).  Handles are synchronised when these calls return and may then be passed to
 * ghicp_register_clouds of ANY context on the same device. */
int ghicp_cloud_recompute(ghicp_cloud* cloud, const float* xyz, int64_t n, int stride);
/* The front ends of n_clouds raw clouds [device pointers xyz[i], n[i] points of `stride` floats] into existing handles of ONE
 * front-end configuration, in one sequence of launches for the whole batch (one radix sort, one cell table, one select ... for all the
 * clouds).  Same results as ghicp_cloud_recompute(clouds[i], xyz[i], n[i], stride) for every i, bit for bit.  (The reference has no
 * counterpart: test/ghicp_main.cpp:86-127 runs the front end once per cloud.) */
int ghicp_clouds_recompute(ghicp_ctx* ctx, int32_t n_clouds, ghicp_cloud* const* clouds, const float* const* xyz /*[host] array of device pointers*/,
                           const int64_t* n /*[host]*/, int stride);
int ghicp_cloud_destroy(ghicp_cloud* cloud);
int ghicp_cloud_get_info(const ghicp_cloud* cloud, ghicp_cloud_info* info /*[host]*/);
/* any destination may be NULL: ds_xyz m x 3 f32, kp_idx k, kp_xyz k x 3 f64, feat feature_bytes */
int ghicp_cloud_download(const ghicp_cloud* cloud, float* ds_xyz, int32_t* kp_idx, double* kp_xyz, void* feat);
/* S[i] -> T[i] for n_pairs pairs of cached clouds; cfg must describe the front end the handles were built with
 * (cfg->reg.corr and the loop parameters may differ from call to call).  stats: n_pairs [host]. */
int ghicp_register_clouds(ghicp_ctx* ctx, const ghicp_pair_config* cfg, int32_t n_pairs, const ghicp_cloud* const* S,
                          const ghicp_cloud* const* T, ghicp_pair_stats* stats);

/* ------------------------------------------------------------------------------------------------
 * Coarse-to-fine over cached clouds: the loop of ghicp_icp for many pairs of handles at once, from the poses ghicp_register_clouds
 * returned.  Same results as, per pair, ghicp_cloud_download + ghicp_transform_cloud_f32(source, float(Rt_init)) + ghicp_icp against the
 * target's down-sampled cloud, bit for bit.  (The reference runs icp_reg / ptplicp_reg pair by pair; it has no counterpart.)
 * ------------------------------------------------------------------------------------------------ */
/* Builds what `cloud` needs to serve as a TARGET and keeps it in the handle: the 1-NN search grids over its down-sampled points and, for
 * covariance_k in 1..20, the k-NN normals ghicp_icp computes for ptplicp_reg (0: none).  Calling it again with another k replaces the
 * normals and keeps the grids.  ghicp_cloud_recompute / ghicp_clouds_recompute invalidate the prepared state, ghicp_cloud_destroy frees
 * it.  The handle is synchronised on return.  GHICP_ERR_ARG for a handle rebuilt by ghicp_cloud_from_features (it holds no points). */
int ghicp_cloud_prepare_refine(ghicp_cloud* cloud, int32_t covariance_k);

typedef struct ghicp_refine_result {
  float T_icp[16];        /* ICP's final_transformation_ (row-major), on top of float(Rt_init); identity for a refused pair */
  double Rt_refined[16];  /* double(T_icp) * double(float(Rt_init)), f64 on the host: the refined source->target pose */
  ghicp_icp_stats stats;  /* as ghicp_icp fills it; done = 0: refused by the overlap gate */
} ghicp_refine_result;

/* S[p] -> T[p] for n_pairs pairs, from Rt_init (n_pairs x 16 row-major f64 [host], the Rt of ghicp_pair_stats; NULL: identity for every
 * pair).  Both metrics, use_trimmed 0 / 1 (with the overlap gate: a refused pair gets done = 0, T_icp = I, Rt_refined = the float-rounded
 * init).  NOT covered by this call: use_reciprocal != 0 -- the reciprocal test needs a grid over the moved source per pair per iteration;
 * it gets GHICP_ERR_ARG here (use ghicp_refine_clouds_reciprocal below, which builds those grids for a whole chunk at once, or ghicp_icp
 * pair by pair).  GHICP_ERR_ARG also for a target that is not prepared, for point-to-plane
 * with normals prepared for a k other than params->covariance_k, and for handles of another device; nothing is written then.  The
 * handles are const: nothing is built lazily, so prepared handles may be shared between contexts of the device.
 * max_concurrent: pairs that share one launch sequence (chunks of that size, in the given order; at most 4096); 0: chosen from the free
 * device memory.  Results do not depend on it.  out: n_pairs [host]. */
int ghicp_refine_clouds(ghicp_ctx* ctx, const ghicp_icp_params* params, int32_t n_pairs, const ghicp_cloud* const* S, const ghicp_cloud* const* T,
                        const double* Rt_init /*[host]*/, int32_t max_concurrent, ghicp_refine_result* out /*[host]*/);
/* ghicp_refine_clouds with params->use_reciprocal honoured (CRegistration::icp_reg / ptplicp_reg's use_reciprocal_correspondence,
 * common_reg.cpp:45-107, 122-199).  Arguments, checks, chunking, results and the preparation required of the targets are those of
 * ghicp_refine_clouds (ghicp_cloud_prepare_refine on targets, nothing extra for sources); the handles are const and nothing is built lazily.
 * use_reciprocal != 0: pair p comes out as ghicp_cloud_download + ghicp_transform_cloud_f32(source, float(Rt_init[p])) + ghicp_icp with
 * use_reciprocal = 1 gives it, bit for bit (T_icp, Rt_refined and every field of stats): per iteration the forward search, in a pair's first
 * iteration the overlap gate from it, then a correspondence i -> j is dropped unless i is the nearest moved source point of target point j
 * (ties to the lower index), then count / trim / solve; the final fitness search has no reciprocal test.  The grids over the moved sources of
 * all running pairs of a chunk are built in one launch sequence per iteration, without a host wait, inside cell tables sized before the
 * loop (about 0.5 KB of device memory per source point of a chunk; max_concurrent = 0 accounts for it).  use_reciprocal == 0: the results of
 * ghicp_refine_clouds, bit for bit (the same code).  The result of a pair does not depend on the other pairs, their order or max_concurrent. */
int ghicp_refine_clouds_reciprocal(ghicp_ctx* ctx, const ghicp_icp_params* params, int32_t n_pairs, const ghicp_cloud* const* S, const ghicp_cloud* const* T,
                                   const double* Rt_init /*[host]*/, int32_t max_concurrent, ghicp_refine_result* out /*[host]*/);

/* ------------------------------------------------------------------------------------------------
 * Generalized ICP over cached clouds: the loop of ghicp_gicp_from for many pairs of handles at once.  (The reference runs gicp_reg pair
 * by pair and without a guess; it has no counterpart.)
 * ------------------------------------------------------------------------------------------------ */
/* Keeps in the handle what `cloud` needs to serve as SOURCE or TARGET of ghicp_gicp_clouds: the m x 6 f64 regularised covariances of its
 * down-sampled points for (covariance_k in 1..20, gicp_epsilon > 0), as ghicp_gicp_covariances gives them (48 B per point), and the 1-NN
 * grids of ghicp_cloud_prepare_refine if the handle does not hold them yet (the same state, built once whichever call comes first).
 * Calling it again with the same values changes nothing; other values replace the covariances and keep grids and normals.
 * ghicp_cloud_prepare_refine keeps the covariances.  ghicp_cloud_recompute / ghicp_clouds_recompute invalidate them, ghicp_cloud_destroy
 * frees them.  The handle is synchronised on return and may then serve any context of the device.  GHICP_ERR_ARG for a handle rebuilt by
 * ghicp_cloud_from_features (it holds no points). */
int ghicp_cloud_prepare_gicp(ghicp_cloud* cloud, int32_t covariance_k, double gicp_epsilon);

typedef struct ghicp_gicp_result {
  float T[16];            /* the final transformation_ (row-major): the total source->target pose; float(Rt_init) for a refused pair */
  ghicp_icp_stats stats;  /* as ghicp_gicp_from fills it; done = 0: refused by the overlap gate */
} ghicp_gicp_result;

/* S[p] -> T[p] for n_pairs pairs, from Rt_init (n_pairs x 16 row-major f64 [host]; NULL: identity for every pair).  Pair p comes out as
 * ghicp_gicp_from(down-sampled S[p], down-sampled T[p], params, float(Rt_init[p])) gives it, bit for bit (T and every field of stats),
 * whatever the other pairs do and whatever max_concurrent is.  A refused pair gets done = 0, T = float(Rt_init[p]) and overlap filled.
 * GHICP_ERR_ARG when a handle of a pair does not hold covariances for (params->covariance_k, params->gicp_epsilon), when a target holds no
 * grids, for a handle without points and for handles of another device; every pair is checked before anything is written or launched.
 * The handles are const.  max_concurrent as in ghicp_refine_clouds.  out: n_pairs [host]. */
int ghicp_gicp_clouds(ghicp_ctx* ctx, const ghicp_gicp_params* params, int32_t n_pairs, const ghicp_cloud* const* S, const ghicp_cloud* const* T,
                      const double* Rt_init /*[host] n_pairs x 16, NULL = identity*/, int32_t max_concurrent, ghicp_gicp_result* out /*[host]*/);

/* ghicp_gicp_clouds with the trimmed rejector applied: pair p comes out as ghicp_gicp_trimmed_from(down-sampled S[p], down-sampled T[p],
 * params, float(Rt_init[p]), trim_ratio) gives it, bit for bit (T and every field of stats), whatever the other pairs do and whatever
 * max_concurrent is.  trim_ratio == 0 (requires params->use_trimmed = 1): every pair keeps the share its OWN gate overlap estimates.
 * Preparation, argument checks, refusal and chunking are those of ghicp_gicp_clouds, plus GHICP_ERR_ARG for a trim_ratio that is negative,
 * above 1 or not finite, or 0 without use_trimmed.  48 KB of histograms per pair of a chunk on top of ghicp_gicp_clouds' buffers. */
int ghicp_gicp_clouds_trimmed(ghicp_ctx* ctx, const ghicp_gicp_params* params, int32_t n_pairs, const ghicp_cloud* const* S, const ghicp_cloud* const* T,
                              const double* Rt_init /*[host] n_pairs x 16, NULL = identity*/, float trim_ratio, int32_t max_concurrent,
                              ghicp_gicp_result* out /*[host]*/);

/* ------------------------------------------------------------------------------------------------
 * calOverlap over cached clouds: which of MANY pairs of handles overlap at all under given poses -- CRegistration::calOverlap
 * (src/common_reg.cpp:294-317) for every pair of a list in one launch per chunk, before registration (poses from odometry or GNSS), between
 * coarse and fine registration (drop the pairs whose GH-ICP pose is wrong) or afterwards (edge weights of the scan graph).  (The reference
 * runs calOverlap pair by pair inside icp_reg / gicp_reg; it has no counterpart.)
 * ------------------------------------------------------------------------------------------------ */
/* Keeps in the handle the search grid of cell thre_dis over its down-sampled points (what ghicp_cal_overlap builds for its
 * second cloud on every call).  Same thre_dis again: nothing happens; another thre_dis replaces the grid.
 * ghicp_cloud_prepare_refine / ghicp_cloud_prepare_gicp keep it and it leaves their state alone; ghicp_cloud_recompute / ghicp_clouds_recompute
 * invalidate it, ghicp_cloud_destroy frees it.  The handle is synchronised on return and may then serve any context of the device.
 * GHICP_ERR_ARG for thre_dis <= 0 and for a handle rebuilt by ghicp_cloud_from_features (it holds no points). */
int ghicp_cloud_prepare_overlap(ghicp_cloud* cloud, float thre_dis);

typedef struct ghicp_overlap_result {
  int64_t hits;     /* source points with a target point at d^2 < thre_dis^2 */
  int64_t n;        /* down-sampled points of the source */
  float ratio;      /* (float)((0.01 + hits) / (double)n), common_reg.cpp:313; 0 when n == 0 */
  int32_t pad_;
} ghicp_overlap_result;

/* S[p] in T[p] for n_pairs pairs under Rt (source->target).  hits and ratio of pair p equal, bit for bit, what
 * ghicp_transform_cloud_f32(down-sampled S[p], float(Rt[p])) followed by ghicp_cal_overlap(that, down-sampled T[p], thre_dis) gives --
 * whatever the other pairs are, whatever their order, whatever max_concurrent is.  Empty source: hits = 0, ratio = 0; empty target:
 * hits = 0, ratio = 0.01 / n (neither launches anything).  The moved source is not stored.
 * GHICP_ERR_ARG: a target that is not prepared, or prepared for another thre_dis (the floats are compared exactly); a source or target
 * rebuilt by ghicp_cloud_from_features; a handle of another device; thre_dis <= 0.  Every pair is checked before anything is written or
 * launched: `out` is untouched then.  Sources need no preparation.  The handles are const: nothing is built lazily, so a prepared handle
 * may serve any context of the device.
 * max_concurrent: pairs per launch (chunks of that size, in the given order; at most 4096); 0: chosen by the library. */
int ghicp_overlap_clouds(ghicp_ctx* ctx, float thre_dis, int32_t n_pairs, const ghicp_cloud* const* S, const ghicp_cloud* const* T,
                         const double* Rt /*[host] n_pairs x 16 row-major source->target, NULL = identity*/,
                         int32_t max_concurrent, ghicp_overlap_result* out /*[host]*/);

/* all ordered pairs of n_clouds handles under cloud->world poses (n_clouds x 16 f64 [host], NULL = all identity):
 * out[i * n_clouds + j] = ratio of cloud i in cloud j under inv(P_j) * P_i; the diagonal is not computed and is 1.
 * Argument checks, the pose products on the host and ONE ghicp_overlap_clouds call (NULL poses: with Rt = NULL).  Every handle must be
 * prepared for thre_dis, because every handle is a target; n_clouds <= 32768; GHICP_ERR_ARG otherwise, `out` untouched.
 * The pair pose is the RIGID inverse, in f64, with P = [R t; 0 0 0 1] row-major (R[r][c] = P[4 r + c], t[r] = P[4 r + 3]):
 *   Rt[r][c] = (R_j[0][r] * R_i[0][c] + R_j[1][r] * R_i[1][c]) + R_j[2][r] * R_i[2][c]                         = (R_j^T R_i)[r][c]
 *   Rt[r][3] = (R_j[0][r] * (t_i[0] - t_j[0]) + R_j[1][r] * (t_i[1] - t_j[1])) + R_j[2][r] * (t_i[2] - t_j[2])  = (R_j^T (t_i - t_j))[r]
 * every sum of three terms added left to right, no fused multiply-add, bottom row 0 0 0 1; ghicp_overlap_clouds then rounds it to float.
 * (NOT ghicp_inv_transform, which keeps the reference's negated-translation quirk.) */
int ghicp_overlap_matrix(ghicp_ctx* ctx, float thre_dis, int32_t n_clouds, const ghicp_cloud* const* clouds, const double* poses,
                         float* out /*[host] n_clouds x n_clouds*/);

/* ------------------------------------------------------------------------------------------------
 * Batched prepare: what ghicp_cloud_prepare_refine / ghicp_cloud_prepare_gicp / ghicp_cloud_prepare_overlap build cloud by cloud, for MANY
 * handles in one launch sequence per chunk -- every recompute invalidates the prepared state, so a streaming caller pays for it with every
 * batch of scans.  (The reference builds its kd-trees, normals and covariances inside every icp_reg / ptplicp_reg / gicp_reg call; it has
 * no counterpart.)
 * ------------------------------------------------------------------------------------------------ */
typedef struct ghicp_prepare_spec {
  int32_t refine;       /* != 0: fine + coarse 1-NN grids (ghicp_cloud_prepare_refine) */
  int32_t normals_k;    /* 0..20; > 0 implies refine: the k-NN normals of ghicp_cloud_prepare_refine(c, normals_k) */
  int32_t gicp_k;       /* 0: none; 1..20 implies refine: the covariances of ghicp_cloud_prepare_gicp(c, gicp_k, gicp_epsilon) */
  int32_t overlap;      /* != 0: the grid of ghicp_cloud_prepare_overlap(c, thre_dis) */
  float   thre_dis;     /* > 0 when overlap */
  int32_t pad_;
  double  gicp_epsilon; /* > 0 when gicp_k */
} ghicp_prepare_spec;
/* all zero, gicp_epsilon 1e-3, thre_dis 0.5; GHICP_ERR_ARG for NULL */
int ghicp_prepare_spec_default(ghicp_prepare_spec* s);
/* After the call every handle of the list is in exactly the state these per-cloud calls leave, made in this order, bit for bit (every
 * descriptor, every buffer):
 *   1. ghicp_cloud_prepare_refine(c, normals_k)        when refine != 0 or normals_k > 0
 *   2. ghicp_cloud_prepare_gicp(c, gicp_k, gicp_epsilon) when gicp_k > 0  (it builds the 1-NN grids itself when the handle holds none; alone it
 *                                                      leaves the normals and their k as they are, as the per-cloud call does)
 *   3. ghicp_cloud_prepare_overlap(c, thre_dis)        when overlap != 0
 * with their keep / replace rules: state held for the same parameters is not rebuilt, another k replaces the normals and keeps the grids,
 * normals_k = 0 with refine keeps the normals' buffer and sets their k to 0, and so on.  A handle's result depends neither on the other
 * handles of the list nor on their order.  The list goes through in chunks of at most 64 clouds (fewer when the points of a chunk would
 * reach 2^31 - 2 or the cells of one of its grids 2^28); per chunk ONE launch sequence, and host waits whose number does not grow with the
 * clouds of the chunk: one for the bounding boxes of the whole list, one per halving round of the fine cell (at most five, for all clouds
 * still halving), one at the end.  One k-NN search serves normals and covariances when normals_k == gicp_k; otherwise two searches run.
 * Handles are synchronised on return and may then serve any context of the device.
 * Every handle and the spec are checked before anything is touched or launched; GHICP_ERR_ARG then leaves every handle as it was: a NULL
 * handle, a handle listed twice, a handle rebuilt by ghicp_cloud_from_features, a handle of another context than ctx (the rule of
 * ghicp_clouds_recompute), normals_k or gicp_k outside 0..20, thre_dis <= 0 with overlap, gicp_epsilon <= 0 with gicp_k.  n_clouds == 0 or
 * a spec that asks for nothing: GHICP_OK, nothing happens.  In host-pointer mode the per-cloud calls run one after the other. */
int ghicp_clouds_prepare(ghicp_ctx* ctx, int32_t n_clouds, ghicp_cloud* const* clouds /*[host]*/, const ghicp_prepare_spec* spec);
/* host waits (stream synchronisations) of the last ghicp_clouds_prepare of this context */
int ghicp_ctx_prepare_host_waits(const ghicp_ctx* ctx, int64_t* waits);

/* Reading the prepared state back: the normals and covariances of the down-sampled cloud without computing them again, and how the two
 * ways of preparing are compared. */
typedef struct ghicp_grid_info { float mn[3]; float inv; int32_t dim[3]; int32_t n; uint32_t ncell; int32_t pad_; } ghicp_grid_info;
typedef struct ghicp_cloud_prepared {
  int32_t refine_ready, normals_k, gicp_ready, gicp_k, overlap_ready, pad_;
  float thre_dis, pad2_; double gicp_epsilon;
  ghicp_grid_info fine, coarse, overlap;           /* zeroed when not held */
} ghicp_cloud_prepared;
int ghicp_cloud_get_prepared(const ghicp_cloud* cloud, ghicp_cloud_prepared* out /*[host]*/);
enum { GHICP_PREP_FINE_PTS, GHICP_PREP_FINE_START, GHICP_PREP_COARSE_PTS, GHICP_PREP_COARSE_START,
       GHICP_PREP_OVERLAP_PTS, GHICP_PREP_OVERLAP_START, GHICP_PREP_NORMALS, GHICP_PREP_COVARIANCES };
/* *_PTS: m x 4 f32 in cell order (w = the bits of the point's index in the down-sampled cloud, copied as bytes); *_START: ncell + 1 u32;
 * normals m x 3 f32; covariances m x 6 f64.  `out` follows the context's pointer mode, like ghicp_cloud_download.  GHICP_ERR_ARG when that
 * part is not held (normals: prepared with k = 0). */
int ghicp_cloud_download_prepared(const ghicp_cloud* cloud, int32_t which, void* out);

/* ------------------------------------------------------------------------------------------------
 * Pair queue: independent scan pairs sharded over the GPUs of ONE node, one process per GPU (BASELINE configs[3]).
 * The reference registers one pair per process run (test/ghicp_main.cpp:56-160) and has no counterpart; a caller of the drop-in
 * headers that holds MANY pairs shards them with these calls.  Pairs share nothing, so there is NO collective on the data path --
 * what the ranks exchange is
 *   - the pair manifest (scene ids / paths / parameters, a few KB): ghicp_pairqueue_broadcast  = one ncclBroadcast,
 *   - per step, every rank's block of result records:               ghicp_pairqueue_gather_records = one ncclAllGather,
 *   - for the dynamic split, claims on one shared counter:          ghicp_pairqueue_claim (an atomic add in host shared memory).
 * Transports: GHICP_PQ_RCCL -- an RCCL communicator over xGMI (librccl is opened when the first such queue is created; the
 * ncclUniqueId travels through the rendezvous segment); GHICP_PQ_HOST -- the same three operations through the rendezvous segment
 * alone (ranks that share a GPU, which RCCL refuses, and the world-size-2 tests on a machine without one).
 * `rendezvous`: path of a file every rank of the job can map (e.g. under /dev/shm), new for every queue; rank 0 creates it, the
 * others wait for it (up to timeout_s seconds).  All buffers of these calls are HOST memory.  Collective calls (create, broadcast,
 * gather_records, barrier, counter_reset, destroy) must be made by every rank, in the same order. */
enum { GHICP_PQ_HOST = 0, GHICP_PQ_RCCL = 1 };
enum { GHICP_PQ_RECORD_WIDTH = 19 }; /* pair id, iterations, converged, the 16 entries of the 4x4 (row-major); pair id -1: unused row */
typedef struct ghicp_pairqueue ghicp_pairqueue;
/* ctx: the rank's context (its device and stream carry the RCCL transfers); may be NULL for GHICP_PQ_HOST. */
int ghicp_pairqueue_create(ghicp_ctx* ctx, const char* rendezvous, int32_t rank, int32_t world, int32_t transport, double timeout_s,
                           ghicp_pairqueue** queue);
int ghicp_pairqueue_destroy(ghicp_pairqueue* queue);
const char* ghicp_pairqueue_last_error(const ghicp_pairqueue* queue);
int ghicp_pairqueue_info(const ghicp_pairqueue* queue, int32_t* rank, int32_t* world, int32_t* transport);
/* `bytes` bytes of root's `buf` into every rank's `buf`. */
int ghicp_pairqueue_broadcast(ghicp_pairqueue* queue, void* buf, int64_t bytes, int32_t root);
int ghicp_pairqueue_barrier(ghicp_pairqueue* queue);
/* Static split: pair p belongs to rank p mod world.  ids: capacity `cap`; *n = number of pairs of this rank (ascending). */
int ghicp_pairqueue_static_share(const ghicp_pairqueue* queue, int64_t n_pairs, int64_t* ids, int64_t cap, int64_t* n);
/* Dynamic split: the next `count` pair ids below `limit` from the queue's shared counter: [*first, *first + *n), *n == 0 when the job
 * is drained.  Not collective.  ghicp_pairqueue_counter_reset (collective) starts the next job at 0. */
int ghicp_pairqueue_claim(ghicp_pairqueue* queue, int64_t count, int64_t limit, int64_t* first, int64_t* n);
int ghicp_pairqueue_counter_reset(ghicp_pairqueue* queue);
/* Every rank's `rows` x GHICP_PQ_RECORD_WIDTH block (f64) into all[world x rows x GHICP_PQ_RECORD_WIDTH] on every rank, rank order. */
int ghicp_pairqueue_gather_records(ghicp_pairqueue* queue, const double* block, int64_t rows, double* all);
/* ghicp_pair_stats of this rank's pairs -> record rows (pair ids in `ids`); rows beyond n_mine get pair id -1. */
int ghicp_pairqueue_pack_records(const int64_t* ids, const ghicp_pair_stats* stats, int64_t n_mine, int64_t rows, double* block);
/* ghicp_register_pairs of THIS RANK'S SHARE of n_pairs pairs (static split when chunk <= 0, else claims of `chunk` pairs from the
 * shared counter), then one gather: records[n_pairs x GHICP_PQ_RECORD_WIDTH] of ALL pairs, in pair order, on every rank.  xyzS / xyzT /
 * nS / nT are indexed by GLOBAL pair id; a rank only touches the entries of the pairs it registers (device pointers, like
 * ghicp_register_pairs).  stats (n_pairs, [host], may be NULL): filled for this rank's pairs only.  Collective. */
int ghicp_pairqueue_register_pairs(ghicp_pairqueue* queue, ghicp_ctx* ctx, const ghicp_pair_config* cfg, int64_t n_pairs, const float* const* xyzS,
                                   const int64_t* nS, const float* const* xyzT, const int64_t* nT, int stride, int64_t chunk,
                                   ghicp_pair_stats* stats, double* records);

/* StereoBinaryFeature::writeFeatures / readFeatures (src/stereo_binary_feature.cpp:107-148): the reference's dump
 * format for one vector of 441-bit strings.  Host memory.  ghicp_sbf_read with feat == NULL only reports *k. */
int ghicp_sbf_write(const char* path, const uint8_t* feat /*k x 56*/, int64_t k);
int ghicp_sbf_read(const char* path, uint8_t* feat /*capacity x 56 or NULL*/, int64_t capacity, int64_t* k);

#ifdef __cplusplus
}
#endif
#endif /* GHICP_C_H_ */
