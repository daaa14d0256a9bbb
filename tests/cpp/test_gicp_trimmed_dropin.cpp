// A reference-style caller of CRegistration<pcl::PointXYZ>::trimmed_gicp_reg (the drop-in's gicp_reg with the trimmed rejector applied; the
// reference announces it and has no counterpart) through the drop-in headers: reads two clouds (int32 n, then n x 3 float), runs
// trimmed_gicp_reg with gicp_reg's arguments, and prints the result for the pytest wrapper (tests/test_gpu_gicp_trimmed.py):
// "RESULT ok iterations reason n correspondences overlap", the 4x4 row by row, and the output cloud as "OUT" rows.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "common_reg.h"

using namespace ghicp;
typedef pcl::PointXYZ Point_T;

static pcl::PointCloud<Point_T>::Ptr load(const char* path) {
  pcl::PointCloud<Point_T>::Ptr c(new pcl::PointCloud<Point_T>());
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  int n = 0;
  if (fread(&n, 4, 1, f) != 1) exit(2);
  c->points.resize(n);
  for (int i = 0; i < n; i++) {
    float p[3];
    if (fread(p, 4, 3, f) != 3) exit(2);
    c->points[i].x = p[0]; c->points[i].y = p[1]; c->points[i].z = p[2];
  }
  fclose(f);
  return c;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  pcl::PointCloud<Point_T>::Ptr S = load(argv[1]), T = load(argv[2]);
  pcl::PointCloud<Point_T>::Ptr out(new pcl::PointCloud<Point_T>());
  Eigen::Matrix4f S2T;
  CRegistration<Point_T> reg;
  // max_iter, use_reciprocal_correspondence, use_trimmed_rejector, thre_dis, covariance_K, min_overlap_for_reg
  const bool ok = reg.trimmed_gicp_reg(S, T, out, S2T, 40, false, true, 0.3f, 20, 0.1f);
  printf("RESULT %d %d %d %zu %lld %.9g\n", ok ? 1 : 0, reg.last_stats.iterations, reg.last_stats.reason, out->points.size(),
         (long long)reg.last_stats.correspondences, reg.last_stats.overlap);
  for (int r = 0; r < 4; r++) printf("ROW %.9g %.9g %.9g %.9g\n", S2T(r, 0), S2T(r, 1), S2T(r, 2), S2T(r, 3));
  for (size_t i = 0; i < out->points.size(); i++) printf("OUT %.9g %.9g %.9g\n", out->points[i].x, out->points[i].y, out->points[i].z);
  return 0;
}
