// TEST INFRASTRUCTURE: single-threaded CPU restatement of the generalized ICP that APPLIES the trimmed rejector (ghicp_gicp_trimmed_from),
// under the contract of include/ghicp_c.h and DESIGN.md §4a, written from that text and not from the kernels.  It is the loop of gcpu_gicp
// (gicp_cpu.cpp, included below for its covariances, Mahalanobis matrices, Gauss-Newton sums and solve) with two additions: transformation_
// starts at a guess, and every outer iteration keeps, of the `count` correspondences within the distance, the
// nv = min(count, floor(ratio * float(count))) smallest by the key (float d^2 bits, source index) -- found here by an actual sort.
// Built by tests/gicp_trimmed_restatement.py like gicp_cpu.cpp.
#include "gicp_cpu.cpp"

#include <cstdint>
#include <utility>

extern "C" {

// Returns 1 when it ran, 0 when refused by the overlap gate.  guess16: row-major float 4x4 or NULL (identity).  trim_ratio in (0, 1], or 0:
// the overlap the gate estimated (the caller sets use_trimmed then).
int gcpu_gicp_trimmed(const float* src, int ns, int ss, const float* tgt, int nt, int ts, const Params* P, const float* guess16, float trim_ratio,
                      float* T16, float* transformed, Stats* st) {
  std::memset(st, 0, sizeof(*st));
  float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  if (guess16) std::memcpy(T, guess16, sizeof(T));
  float ratio = trim_ratio;
  if (P->use_trimmed) {  // the gate sees the source where the guess puts it
    std::vector<float> moved((size_t)ns * 3);
    for (int i = 0; i < ns; i++) xform(T, &src[(size_t)i * ss], &moved[(size_t)i * 3]);
    st->overlap = guess16 ? orc_cal_overlap(moved.data(), ns, 3, tgt, nt, ts, P->thre_dis) : orc_cal_overlap(src, ns, ss, tgt, nt, ts, P->thre_dis);
    if (st->overlap < P->min_overlap) return 0;
    if (trim_ratio == 0.f) ratio = st->overlap;
  }
  st->done = 1;
  if (ns == 0 || nt == 0) {
    st->reason = 5;
  } else {
    std::vector<double> covS((size_t)ns * 6), covT((size_t)nt * 6), M6((size_t)ns * 6);
    covariances(src, ns, ss, P->covariance_k, P->gicp_epsilon, covS.data());
    covariances(tgt, nt, ts, P->covariance_k, P->gicp_epsilon, covT.data());
    std::vector<float> cur((size_t)ns * 3);
    std::vector<int> nn(ns), si, tj;
    std::vector<float> nd(ns);
    std::vector<std::pair<uint32_t, uint32_t>> keys;
    std::vector<char> kept(ns);
    const double maxd2 = P->max_correspondence_distance * P->max_correspondence_distance;
    for (;;) {
      for (int i = 0; i < ns; i++) xform(T, &src[(size_t)i * ss], &cur[(size_t)i * 3]);
      orc_nn1(cur.data(), ns, 3, tgt, nt, ts, nn.data(), nd.data());
      double R[9];
      for (int e = 0; e < 9; e++) R[e] = (double)T[(e / 3) * 4 + e % 3];
      // 3. the distance rejection; 4. the trim: the nv smallest keys of the survivors
      keys.clear();
      for (int i = 0; i < ns; i++) {
        if (nn[i] < 0 || !((double)nd[i] < maxd2)) continue;
        uint32_t bits;
        std::memcpy(&bits, &nd[i], 4);
        keys.emplace_back(bits, (uint32_t)i);
      }
      const unsigned count = (unsigned)keys.size();
      unsigned nv = (unsigned)(int)std::floor(ratio * (float)count);  // float product, as CorrespondenceRejectorTrimmed forms it
      if (nv > count) nv = count;
      std::sort(keys.begin(), keys.end());
      std::fill(kept.begin(), kept.end(), 0);
      for (unsigned r = 0; r < nv; r++) kept[keys[r].second] = 1;
      // 5. M_i, count and MSE over the kept set, in source order
      si.clear();
      tj.clear();
      double d2sum = 0;
      for (int i = 0; i < ns; i++) {
        if (!kept[i]) continue;
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
      for (int it = 0; it < P->max_inner_iter; it++) {
        double H[21], g[6], e, dx[6], mx;
        gn_sums(src, ss, tgt, ts, si, tj, M6, x, H, g, &e);
        round_n2(H, 21);
        round_n2(g, 6);
        if (!gn_solve(H, g, dx, &mx)) break;
        for (int p = 0; p < 6; p++) x[p] += dx[p];
        if (mx < 1e-10) break;
      }
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
          const double sc = (r < 3 && c < 3) ? 1.0 / P->rotation_epsilon : 1.0 / P->transformation_epsilon;
          delta = std::max(delta, sc * std::fabs((double)T[r * 4 + c] - (double)Tn[r * 4 + c]));
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
