// A reference-style caller of CFilter<PointT>::SORFilter / DisFilter / ActiveObjectFilter (reference include/filter.hpp:90-140) through
// the drop-in header: reads a cloud (int32 n, then n x 3 float), runs the three filters with the arguments of the command line
//   cloud.bin MeanK std xy_dis_max z_min z_max [min_x min_y min_z max_x max_y max_z]...
// and prints for the pytest wrapper (tests/test_gpu_filters.py) "SOR m", "DIS m", "BOX m" and a checksum line per filter: the sum of the
// kept points' x, y and z in double (the whole point structs travel, so the coordinates must be the inputs').
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "filter.hpp"

using namespace ghicp;
typedef pcl::PointXYZ Point_T;

static void report(const char* tag, const pcl::PointCloud<Point_T>::Ptr& c) {
  double s[3] = {0, 0, 0};
  for (size_t i = 0; i < c->points.size(); i++) { s[0] += c->points[i].x; s[1] += c->points[i].y; s[2] += c->points[i].z; }
  printf("%s %zu\n%sSUM %.17g %.17g %.17g\n", tag, c->points.size(), tag, s[0], s[1], s[2]);
}

int main(int argc, char** argv) {
  if (argc < 7 || (argc - 7) % 6 != 0) return 2;
  pcl::PointCloud<Point_T>::Ptr in(new pcl::PointCloud<Point_T>());
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int n = 0;
  if (fread(&n, 4, 1, f) != 1) return 2;
  in->points.resize(n);
  for (int i = 0; i < n; i++) {
    float p[3];
    if (fread(p, 4, 3, f) != 3) return 2;
    in->points[i].x = p[0]; in->points[i].y = p[1]; in->points[i].z = p[2];
  }
  fclose(f);
  CFilter<Point_T> filter;
  pcl::PointCloud<Point_T>::Ptr sor(new pcl::PointCloud<Point_T>()), dis(new pcl::PointCloud<Point_T>()), box(new pcl::PointCloud<Point_T>());
  sor->points.resize(3);  // pcl::Filter::filter replaces the output cloud
  if (!filter.SORFilter(in, sor, atoi(argv[2]), atof(argv[3]))) return 1;
  report("SOR", sor);
  if (!filter.DisFilter(in, dis, atof(argv[4]), atof(argv[5]), atof(argv[6]))) return 1;
  report("DIS", dis);
  std::vector<Bounds> boxes;
  for (int a = 7; a + 5 < argc; a += 6) {
    Bounds b;
    b.min_x = atof(argv[a]); b.min_y = atof(argv[a + 1]); b.min_z = atof(argv[a + 2]);
    b.max_x = atof(argv[a + 3]); b.max_y = atof(argv[a + 4]); b.max_z = atof(argv[a + 5]);
    boxes.push_back(b);
  }
  if (!filter.ActiveObjectFilter(in, box, boxes)) return 1;
  report("BOX", box);
  return 0;
}
