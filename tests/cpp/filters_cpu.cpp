// TEST INFRASTRUCTURE: CPU restatement of CFilter's cleaning filters (reference include/filter.hpp:90-140) under the contract of
// include/ghicp_c.h and DESIGN.md N9 / Q10 / Q11.  Plain C++17, no dependencies; built by tests/filters_restatement.py with
// -ffp-contract=off.  The neighbour search is brute force: it shares nothing with the library's grid.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {
constexpr long long TILE = 1024;  // N9

// mean distance of point i to its mean_k nearest neighbours: the mean_k + 1 smallest float d2 of the cloud (the query among them),
// sorted, entry 0 dropped, sqrtf summed in ascending order in f64
float mean_distance(const float* xyz, long long n, int stride, int mean_k, long long i, std::vector<float>& d2) {
  const float px = xyz[i * stride], py = xyz[i * stride + 1], pz = xyz[i * stride + 2];
  for (long long j = 0; j < n; j++) {
    const float dx = px - xyz[j * stride], dy = py - xyz[j * stride + 1], dz = pz - xyz[j * stride + 2];
    float d = dx * dx;
    d += dy * dy;
    d += dz * dz;
    d2[(size_t)j] = d;
  }
  std::partial_sort(d2.begin(), d2.begin() + mean_k + 1, d2.end());
  double sum = 0.0;
  for (int t = 1; t <= mean_k; t++) sum += (double)std::sqrt(d2[(size_t)t]);  // std::sqrt(float): float
  return (float)(sum / (double)mean_k);
}

void sums(const float* dist, long long n, int tiled, double* sum, double* sq_sum) {
  double s = 0.0, q = 0.0;
  if (!tiled) {  // PCL's own order
    for (long long i = 0; i < n; i++) {
      s += (double)dist[i];
      q += (double)dist[i] * (double)dist[i];
    }
  } else {  // N9: tiles of 1024 consecutive indices in index order, then the tiles in index order
    for (long long b = 0; b < n; b += TILE) {
      double ts = 0.0, tq = 0.0;
      for (long long i = b; i < std::min(b + TILE, n); i++) {
        const double d = (double)dist[i];
        ts += d;
        tq += d * d;
      }
      s += ts;
      q += tq;
    }
  }
  *sum = s;
  *sq_sum = q;
}
}  // namespace

extern "C" {

void fcpu_knn_mean_distance(const float* xyz, long long n, int stride, int mean_k, float* dist) {
  if (n < (long long)mean_k + 1) {  // PCL: a short result list sets the distance to 0
    for (long long i = 0; i < n; i++) dist[i] = 0.f;
    return;
  }
  std::vector<float> d2((size_t)n);
  for (long long i = 0; i < n; i++) dist[i] = mean_distance(xyz, n, stride, mean_k, i, d2);
}

// the same for the queries [i0, i1) alone against the whole cloud (timing scripts: a slice of a cloud too large for n^2 work); dist: i1 - i0 values
void fcpu_knn_mean_distance_range(const float* xyz, long long n, int stride, int mean_k, long long i0, long long i1, float* dist) {
  std::vector<float> d2((size_t)n);
  for (long long i = i0; i < i1; i++) dist[i - i0] = n < (long long)mean_k + 1 ? 0.f : mean_distance(xyz, n, stride, mean_k, i, d2);
}

// stats4 = mean, stddev, threshold, valid count over n valid distances; tiled = 0: sequential sums, 1: the order of N9
void fcpu_sor_stats(const float* dist, long long n, double std_mul, int tiled, double* stats4) {
  double sum, sq_sum;
  sums(dist, n, tiled, &sum, &sq_sum);
  const double dn = (double)n;
  const double mean = sum / dn;
  const double variance = (sq_sum - sum * sum / dn) / (dn - 1.0);
  const double stddev = std::sqrt(variance);
  stats4[0] = mean;
  stats4[1] = stddev;
  stats4[2] = mean + std_mul * stddev;
  stats4[3] = dn;
}

long long fcpu_sor_filter(const float* xyz, long long n, int stride, int mean_k, double std_mul, int32_t* keep, double* stats4, float* dist_out) {
  stats4[0] = stats4[1] = stats4[2] = std::nan("");
  stats4[3] = 0.0;
  if (n < (long long)mean_k + 1) {  // no valid point, NaN threshold: everything stays
    for (long long i = 0; i < n; i++) keep[i] = (int32_t)i;
    return n;
  }
  std::vector<float> dist((size_t)n);
  fcpu_knn_mean_distance(xyz, n, stride, mean_k, dist.data());
  fcpu_sor_stats(dist.data(), n, std_mul, 1, stats4);
  long long m = 0;
  for (long long i = 0; i < n; i++) {
    if (dist_out) dist_out[i] = dist[(size_t)i];
    if (!((double)dist[(size_t)i] > stats4[2])) keep[m++] = (int32_t)i;
  }
  return m;
}

// filter.hpp:105-117 as written: dis_square = x * x + y + y (float expression, stored in a double)
long long fcpu_dis_filter(const float* xyz, long long n, int stride, double xy_dis_max, double z_min, double z_max, int32_t* keep) {
  long long m = 0;
  for (long long i = 0; i < n; i++) {
    const float x = xyz[i * stride], y = xyz[i * stride + 1], z = xyz[i * stride + 2];
    const double dis_square = x * x + y + y;
    if (dis_square < xy_dis_max * xy_dis_max && z < z_max && z > z_min) keep[m++] = (int32_t)i;
  }
  return m;
}

// filter.hpp:119-140: boxes6 = n_boxes x (min_x, min_y, min_z, max_x, max_y, max_z)
long long fcpu_box_filter(const float* xyz, long long n, int stride, const double* boxes6, int n_boxes, int32_t* keep) {
  long long m = 0;
  for (long long i = 0; i < n; i++) {
    const float x = xyz[i * stride], y = xyz[i * stride + 1], z = xyz[i * stride + 2];
    bool is_static = true;
    for (int j = 0; j < n_boxes; j++) {
      const double* b = boxes6 + (size_t)j * 6;
      if (x > b[0] && x < b[3] && y > b[1] && y < b[4] && z > b[2] && z < b[5]) {
        is_static = false;
        break;
      }
    }
    if (is_static) keep[m++] = (int32_t)i;
  }
  return m;
}
}
