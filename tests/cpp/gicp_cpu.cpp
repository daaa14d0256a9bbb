// TEST INFRASTRUCTURE: single-threaded CPU restatement of CRegistration::gicp_reg (reference src/common_reg.cpp:216-284) under the
// contract of DESIGN.md §2 N8 / §4a, written from that text and not from the kernels.  Built by tests/gicp_restatement.py with
// g++ -O2 -ffp-contract=off; links the CPU oracle (oracle/libghicp_oracle.so) for the exact 1-NN search (orc_nn1) and the overlap
// gate (orc_cal_overlap).  The only code shared with the library is gh_jacobi3 (csrc/devmath.h, N3), which the oracle tests pin.
//   covariances : exact k-NN in the point's own cloud (query included, float L2 ((dx^2 + dy^2) + dz^2), ties -> lower index, sorted
//                 by (d2, index)); f64 mean and 1/k scatter summed in that order; N2 rounding of the 6 entries; Jacobi; the
//                 smallest eigenvalue (first on ties) -> eps, the other two -> 1: C_rc = (u_r u_c + v_r v_c) + eps (w_r w_c)
//   outer loop  : source under transformation_ (float), 1-NN, kept when (double) d^2 < max_dist^2,
//                 M_i = inverse of the upper triangle of R C_S R^T + C_T (cofactors), R = transformation_'s 3x3 in f64
//   inner (GN)  : x0 = (t, atan2(R21, R22), asin(-R20), atan2(R10, R00)); per step the f64 sums J^T M J, J^T M r over the
//                 correspondences in source order, each group rounded by N2, H dx = -g by partial-pivot elimination, x += dx;
//                 stop after max_inner_iter steps, once max |dx| < 1e-10, or (without a step) on a non-finite solve
//   outer step  : T = float(R(x)), float(t); delta test; < 4 correspondences ends the loop unconverged (reason 5)
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "devmath.h"

extern "C" void orc_nn1(const float* q, int nq, int qs, const float* tgt, int nt, int ts, int* idx, float* d2);
extern "C" float orc_cal_overlap(const float* c1, int n1, int s1, const float* c2, int n2, int s2, float thre_dis);

namespace {

struct Params {  // layout of ghicp_gicp_params
  int max_iter, use_reciprocal, use_trimmed, covariance_k;
  float thre_dis, min_overlap;
  int max_inner_iter, pad_;
  double max_correspondence_distance, gicp_epsilon, transformation_epsilon, rotation_epsilon;
};
struct Stats {  // layout of ghicp_icp_stats
  int done, iterations, converged, reason;
  long long correspondences;
  float overlap, pad_;
  double mse, fitness;
};

void round_n2(double* v, int n) {  // N2: nearest multiple of 2^(e - 24), e = frexp exponent of the largest |entry|
  double mx = 0;
  for (int i = 0; i < n; i++) mx = std::max(mx, std::fabs(v[i]));
  if (!(mx > 0) || !(mx <= DBL_MAX)) return;
  int e;
  std::frexp(mx, &e);
  const double q = std::ldexp(1.0, e - 24);
  for (int i = 0; i < n; i++) v[i] = std::nearbyint(v[i] / q) * q;
}

// exact k-NN of every point of a cloud over a uniform grid (ring expansion until the k-th best is closer than the unscanned rings)
void knn_all(const float* xyz, int n, int stride, int k, std::vector<int>& nb, std::vector<int>& cnt) {
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (int i = 0; i < n; i++)
    for (int d = 0; d < 3; d++) { mn[d] = std::min(mn[d], xyz[(size_t)i * stride + d]); mx[d] = std::max(mx[d], xyz[(size_t)i * stride + d]); }
  const double vol = std::max(1e-9, (double)(mx[0] - mn[0] + 1e-3) * (mx[1] - mn[1] + 1e-3) * (mx[2] - mn[2] + 1e-3));
  const double cell = std::max(0.05, std::cbrt(vol / n * 4.0));
  int dim[3];
  for (int d = 0; d < 3; d++) dim[d] = std::max(1, std::min(1024, (int)std::floor((mx[d] - mn[d]) / cell) + 1));
  auto coord = [&](double v, int d) { return std::min(dim[d] - 1, std::max(0, (int)std::floor((v - mn[d]) / cell))); };
  const size_t nc = (size_t)dim[0] * dim[1] * dim[2];
  std::vector<int> start(nc + 1, 0), order(n), key(n);
  for (int i = 0; i < n; i++) {
    const float* p = &xyz[(size_t)i * stride];
    key[i] = (coord(p[0], 0) * dim[1] + coord(p[1], 1)) * dim[2] + coord(p[2], 2);
    start[key[i] + 1]++;
  }
  for (size_t c = 0; c < nc; c++) start[c + 1] += start[c];
  {
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (int i = 0; i < n; i++) order[fill[key[i]]++] = i;
  }
  nb.assign((size_t)n * k, -1);
  cnt.assign(n, 0);
  std::vector<std::pair<float, int>> cand;
  const int rmax = std::max(dim[0], std::max(dim[1], dim[2]));
  for (int i = 0; i < n; i++) {
    const float* q = &xyz[(size_t)i * stride];
    const int c[3] = {coord(q[0], 0), coord(q[1], 1), coord(q[2], 2)};
    cand.clear();
    for (int r = 0; r <= rmax; r++) {
      for (int x = std::max(c[0] - r, 0); x <= std::min(c[0] + r, dim[0] - 1); x++)
        for (int y = std::max(c[1] - r, 0); y <= std::min(c[1] + r, dim[1] - 1); y++)
          for (int z = std::max(c[2] - r, 0); z <= std::min(c[2] + r, dim[2] - 1); z++) {
            if (std::max(std::abs(x - c[0]), std::max(std::abs(y - c[1]), std::abs(z - c[2]))) != r) continue;
            const int ci = (x * dim[1] + y) * dim[2] + z;
            for (int t = start[ci]; t < start[ci + 1]; t++) {
              const int j = order[t];
              const float* p = &xyz[(size_t)j * stride];
              const float dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
              float d2 = dx * dx;
              d2 += dy * dy;
              d2 += dz * dz;
              cand.emplace_back(d2, j);
            }
          }
      if ((int)cand.size() >= k) {
        std::nth_element(cand.begin(), cand.begin() + (k - 1), cand.end());
        const double reach = r * cell * (1.0 - 1e-6);  // every unscanned point is at least this far away
        if ((double)cand[k - 1].first < reach * reach) break;
      }
    }
    std::sort(cand.begin(), cand.end());
    const int kk = std::min(k, (int)cand.size());
    for (int t = 0; t < kk; t++) nb[(size_t)i * k + t] = cand[t].second;
    cnt[i] = kk;
  }
}

void covariances(const float* xyz, int n, int stride, int k, double eps, double* cov6) {
  std::vector<int> nb, cnt;
  knn_all(xyz, n, stride, k, nb, cnt);
  for (int i = 0; i < n; i++) {
    const int kk = cnt[i];
    double m[3] = {0, 0, 0};
    for (int t = 0; t < kk; t++)
      for (int d = 0; d < 3; d++) m[d] += (double)xyz[(size_t)nb[(size_t)i * k + t] * stride + d];
    for (int d = 0; d < 3; d++) m[d] /= kk;
    double S[6] = {0, 0, 0, 0, 0, 0};
    for (int t = 0; t < kk; t++) {
      const float* p = &xyz[(size_t)nb[(size_t)i * k + t] * stride];
      const double a = p[0] - m[0], b = p[1] - m[1], c = p[2] - m[2];
      S[0] += a * a; S[1] += a * b; S[2] += a * c; S[3] += b * b; S[4] += b * c; S[5] += c * c;
    }
    for (int e = 0; e < 6; e++) S[e] /= kk;
    round_n2(S, 6);
    double V[9];
    gh_jacobi3(S[0], S[1], S[2], S[3], S[4], S[5], V);
    int w = 0;
    if (S[3] < S[0]) w = 1;
    if (S[5] < (w == 0 ? S[0] : S[3])) w = 2;
    int u = -1, v = -1;
    for (int c = 0; c < 3; c++) if (c != w) { if (u < 0) u = c; else v = c; }
    const int rr[6] = {0, 0, 0, 1, 1, 2}, cc[6] = {0, 1, 2, 1, 2, 2};
    for (int e = 0; e < 6; e++) {
      const int r = rr[e], c = cc[e];
      cov6[(size_t)i * 6 + e] = (V[r * 3 + u] * V[c * 3 + u] + V[r * 3 + v] * V[c * 3 + v]) + eps * (V[r * 3 + w] * V[c * 3 + w]);
    }
  }
}

void sym(const double* s6, double* M) {
  M[0] = s6[0]; M[1] = s6[1]; M[2] = s6[2];
  M[3] = s6[1]; M[4] = s6[3]; M[5] = s6[4];
  M[6] = s6[2]; M[7] = s6[4]; M[8] = s6[5];
}

// (R C_S R^T + C_T)^-1 from the upper triangle
void mahalanobis(const double* R, const double* cs6, const double* ct6, double* out6) {
  double C[9], RC[9];
  sym(cs6, C);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) RC[r * 3 + c] = (R[r * 3 + 0] * C[0 * 3 + c] + R[r * 3 + 1] * C[1 * 3 + c]) + R[r * 3 + 2] * C[2 * 3 + c];
  const int rr[6] = {0, 0, 0, 1, 1, 2}, cc[6] = {0, 1, 2, 1, 2, 2};
  double A[6];
  for (int e = 0; e < 6; e++) {
    const int r = rr[e], c = cc[e];
    A[e] = ((RC[r * 3 + 0] * R[c * 3 + 0] + RC[r * 3 + 1] * R[c * 3 + 1]) + RC[r * 3 + 2] * R[c * 3 + 2]) + ct6[e];
  }
  const double a = A[0], b = A[1], c = A[2], d = A[3], e = A[4], f = A[5];
  const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d, c11 = a * f - c * c, c12 = b * c - a * e, c22 = a * d - b * b;
  const double det = (a * c00 + b * c01) + c * c02;
  out6[0] = c00 / det; out6[1] = c01 / det; out6[2] = c02 / det; out6[3] = c11 / det; out6[4] = c12 / det; out6[5] = c22 / det;
}

// R(x) = Rz(yaw) Ry(pitch) Rx(roll) and the derivatives by roll, pitch, yaw (written out from the product)
void rotation(const double* x, double* R, double* Ra, double* Rb, double* Rg) {
  const double a = x[3], b = x[4], g = x[5];
  const double ca = std::cos(a), sa = std::sin(a), cb = std::cos(b), sb = std::sin(b), cg = std::cos(g), sg = std::sin(g);
  const double Rv[9] = {cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa, sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa, -sb, cb * sa, cb * ca};
  // d/droll: only the columns 1, 2 depend on roll
  const double Av[9] = {0, cg * sb * ca + sg * sa, -cg * sb * sa + sg * ca, 0, sg * sb * ca - cg * sa, -sg * sb * sa - cg * ca, 0, cb * ca, -cb * sa};
  const double Bv[9] = {-cg * sb, cg * cb * sa, cg * cb * ca, -sg * sb, sg * cb * sa, sg * cb * ca, -cb, -sb * sa, -sb * ca};
  const double Gv[9] = {-sg * cb, -sg * sb * sa - cg * ca, -sg * sb * ca + cg * sa, cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa, 0, 0, 0};
  std::memcpy(R, Rv, sizeof(Rv));
  if (Ra) { std::memcpy(Ra, Av, sizeof(Av)); std::memcpy(Rb, Bv, sizeof(Bv)); std::memcpy(Rg, Gv, sizeof(Gv)); }
}

// sums of one Gauss-Newton step over the correspondences (src index order): H = J^T M J (upper, row by row), g = J^T M r, e = r^T M r
void gn_sums(const float* src, int ss, const float* tgt, int ts, const std::vector<int>& si, const std::vector<int>& tj, const std::vector<double>& M6,
             const double* x, double* H21, double* g6, double* e) {
  double R[9], D[3][9];
  rotation(x, R, D[0], D[1], D[2]);
  for (int q = 0; q < 21; q++) H21[q] = 0;
  for (int q = 0; q < 6; q++) g6[q] = 0;
  *e = 0;
  for (size_t c = 0; c < si.size(); c++) {
    const float* sp = &src[(size_t)si[c] * ss];
    const float* tp = &tgt[(size_t)tj[c] * ts];
    const double s[3] = {sp[0], sp[1], sp[2]};
    double r[3], J[3][6];
    for (int q = 0; q < 3; q++) {
      r[q] = (((R[q * 3] * s[0] + R[q * 3 + 1] * s[1]) + R[q * 3 + 2] * s[2]) + x[q]) - (double)tp[q];
      for (int p = 0; p < 3; p++) J[q][p] = (q == p) ? 1.0 : 0.0;
      for (int a = 0; a < 3; a++) J[q][3 + a] = (D[a][q * 3] * s[0] + D[a][q * 3 + 1] * s[1]) + D[a][q * 3 + 2] * s[2];
    }
    double M[9];
    sym(&M6[c * 6], M);
    double Mr[3], MJ[3][6];
    for (int q = 0; q < 3; q++) {
      Mr[q] = (M[q * 3] * r[0] + M[q * 3 + 1] * r[1]) + M[q * 3 + 2] * r[2];
      for (int p = 0; p < 6; p++) MJ[q][p] = (M[q * 3] * J[0][p] + M[q * 3 + 1] * J[1][p]) + M[q * 3 + 2] * J[2][p];
    }
    int k = 0;
    for (int p = 0; p < 6; p++)
      for (int q = p; q < 6; q++) H21[k++] += (J[0][p] * MJ[0][q] + J[1][p] * MJ[1][q]) + J[2][p] * MJ[2][q];
    for (int p = 0; p < 6; p++) g6[p] += (J[0][p] * Mr[0] + J[1][p] * Mr[1]) + J[2][p] * Mr[2];
    *e += (r[0] * Mr[0] + r[1] * Mr[1]) + r[2] * Mr[2];
  }
}

// H dx = -g, partial-pivot elimination; false when the result is not finite
bool gn_solve(const double* H21, const double* g6, double* dx, double* mx) {
  double A[6][6], b[6];
  int k = 0;
  for (int r = 0; r < 6; r++)
    for (int q = r; q < 6; q++) A[r][q] = A[q][r] = H21[k++];
  for (int r = 0; r < 6; r++) b[r] = -g6[r];
  for (int c = 0; c < 6; c++) {
    int piv = c;
    for (int r = c + 1; r < 6; r++) if (std::fabs(A[r][c]) > std::fabs(A[piv][c])) piv = r;
    if (piv != c) { for (int q = 0; q < 6; q++) std::swap(A[c][q], A[piv][q]); std::swap(b[c], b[piv]); }
    for (int r = c + 1; r < 6; r++) {
      const double f = A[r][c] / A[c][c];
      for (int q = c; q < 6; q++) A[r][q] -= f * A[c][q];
      b[r] -= f * b[c];
    }
  }
  *mx = 0;
  for (int r = 5; r >= 0; r--) {
    double s = b[r];
    for (int q = r + 1; q < 6; q++) s -= A[r][q] * dx[q];
    dx[r] = s / A[r][r];
    *mx = std::max(*mx, std::fabs(dx[r]));
  }
  return *mx <= 1e300;
}

void xform(const float* T, const float* p, float* o) {
  const float x = p[0], y = p[1], z = p[2];
  o[0] = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
  o[1] = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
  o[2] = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}

}  // namespace

extern "C" {

void gcpu_covariances(const float* xyz, int n, int stride, int k, double eps, double* cov6) {
  if (n > 0) covariances(xyz, n, stride, k, eps, cov6);
}

// the correspondences of one outer iteration under T16 (row-major float): src index, tgt index, M (6 per correspondence); returns c
int gcpu_correspondences(const float* src, int ns, int ss, const float* tgt, int nt, int ts, const double* covS, const double* covT, const float* T16,
                         double maxd2, int* si, int* tj, double* M6) {
  std::vector<float> cur((size_t)ns * 3);
  for (int i = 0; i < ns; i++) xform(T16, &src[(size_t)i * ss], &cur[(size_t)i * 3]);
  std::vector<int> nn(ns);
  std::vector<float> nd(ns);
  orc_nn1(cur.data(), ns, 3, tgt, nt, ts, nn.data(), nd.data());
  double R[9];
  for (int e = 0; e < 9; e++) R[e] = (double)T16[(e / 3) * 4 + e % 3];
  int c = 0;
  for (int i = 0; i < ns; i++) {
    if (nn[i] < 0 || !((double)nd[i] < maxd2)) continue;
    si[c] = i;
    tj[c] = nn[i];
    mahalanobis(R, &covS[(size_t)i * 6], &covT[(size_t)nn[i] * 6], &M6[(size_t)c * 6]);
    c++;
  }
  return c;
}

// the un-rounded sums of one Gauss-Newton step at x (the Jacobian / gradient test): H21, g6, e
void gcpu_gn_sums(const float* src, int ss, const float* tgt, int ts, int c, const int* si, const int* tj, const double* M6, const double* x,
                  double* H21, double* g6, double* e) {
  std::vector<int> a(si, si + c), b(tj, tj + c);
  std::vector<double> m(M6, M6 + (size_t)c * 6);
  gn_sums(src, ss, tgt, ts, a, b, m, x, H21, g6, e);
}

// gicp_reg.  Returns 1 when it ran, 0 when refused by the overlap gate.  inner_trace (max_iter ints or NULL): steps per iteration.
int gcpu_gicp(const float* src, int ns, int ss, const float* tgt, int nt, int ts, const Params* P, float* T16, float* transformed, Stats* st,
              int* inner_trace) {
  std::memset(st, 0, sizeof(*st));
  if (P->use_trimmed) {  // overlap gate only; GICP never consults the rejector (common_reg.cpp:213-215)
    st->overlap = orc_cal_overlap(src, ns, ss, tgt, nt, ts, P->thre_dis);
    if (st->overlap < P->min_overlap) return 0;
  }
  st->done = 1;
  float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  if (ns == 0 || nt == 0) {
    st->reason = 5;
  } else {
    std::vector<double> covS((size_t)ns * 6), covT((size_t)nt * 6), M6((size_t)ns * 6);
    covariances(src, ns, ss, P->covariance_k, P->gicp_epsilon, covS.data());
    covariances(tgt, nt, ts, P->covariance_k, P->gicp_epsilon, covT.data());
    std::vector<float> cur((size_t)ns * 3);
    std::vector<int> nn(ns), si, tj;
    std::vector<float> nd(ns);
    const double maxd2 = P->max_correspondence_distance * P->max_correspondence_distance;
    for (;;) {
      for (int i = 0; i < ns; i++) xform(T, &src[(size_t)i * ss], &cur[(size_t)i * 3]);
      orc_nn1(cur.data(), ns, 3, tgt, nt, ts, nn.data(), nd.data());
      double R[9];
      for (int e = 0; e < 9; e++) R[e] = (double)T[(e / 3) * 4 + e % 3];
      si.clear();
      tj.clear();
      double d2sum = 0;
      for (int i = 0; i < ns; i++) {
        if (nn[i] < 0 || !((double)nd[i] < maxd2)) continue;
        mahalanobis(R, &covS[(size_t)i * 6], &covT[(size_t)nn[i] * 6], &M6[si.size() * 6]);
        si.push_back(i);
        tj.push_back(nn[i]);
        d2sum += (double)nd[i];
      }
      st->correspondences = (long long)si.size();
      st->mse = si.empty() ? 0.0 : d2sum / (double)si.size();
      if (si.size() < 4) { st->reason = 5; st->converged = 0; break; }
      double x[6] = {T[3], T[7], T[11], std::atan2((double)T[9], (double)T[10]), std::asin(std::min(1.0, std::max(-1.0, -(double)T[8]))),
                     std::atan2((double)T[4], (double)T[0])};
      int steps = 0;
      for (int it = 0; it < P->max_inner_iter; it++) {
        double H[21], g[6], e, dx[6], mx;
        gn_sums(src, ss, tgt, ts, si, tj, M6, x, H, g, &e);
        round_n2(H, 21);
        round_n2(g, 6);
        steps++;
        if (!gn_solve(H, g, dx, &mx)) break;
        for (int p = 0; p < 6; p++) x[p] += dx[p];
        if (mx < 1e-10) break;
      }
      if (inner_trace && st->iterations < P->max_iter) inner_trace[st->iterations] = steps;
      double Rx[9];
      rotation(x, Rx, nullptr, nullptr, nullptr);
      float Tn[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
      for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Tn[r * 4 + c] = (float)Rx[r * 3 + c];
        Tn[r * 4 + 3] = (float)x[r];
      }
      double delta = 0;
      for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
          const double ratio = (r < 3 && c < 3) ? 1.0 / P->rotation_epsilon : 1.0 / P->transformation_epsilon;
          delta = std::max(delta, ratio * std::fabs((double)T[r * 4 + c] - (double)Tn[r * 4 + c]));
        }
      std::memcpy(T, Tn, sizeof(T));
      st->iterations++;
      if (st->iterations >= P->max_iter) { st->converged = 1; st->reason = 1; break; }
      if (delta < 1.0) { st->converged = 1; st->reason = 2; break; }
    }
  }
  std::memcpy(T16, T, sizeof(T));
  std::vector<float> out((size_t)ns * 3);
  for (int i = 0; i < ns; i++) xform(T, &src[(size_t)i * ss], &out[(size_t)i * 3]);
  if (ns > 0 && nt > 0) {
    std::vector<int> nn(ns);
    std::vector<float> nd(ns);
    orc_nn1(out.data(), ns, 3, tgt, nt, ts, nn.data(), nd.data());
    double f = 0;
    for (int i = 0; i < ns; i++) f += (double)nd[i];
    st->fitness = f / ns;
  }
  if (transformed) std::memcpy(transformed, out.data(), out.size() * sizeof(float));
  return 1;
}

}  // extern "C"
