// Internal, host side: one chunk of a batched refiner over cached clouds in flight (RfChunk), for ICP (refine.hip) and generalized ICP
// (refine_gicp.hip).  The chunk owns what the two loops have in common -- the per-pair set-up with ghicp_icp's answers for an empty cloud, the
// reservations, the uploads, the 1-NN search, the overlap gate, the status record, the final search with its fitness sum, the read-back --
// and asks the method M for what differs:
//   Args, Result, Params, TIMER           its argument block (refine_dev.h), its result and parameter structs, its stage timer
//   pair(a, b, D, st, R)                  the pair's loop state, its own descriptor fields, the pose a refused pair reports
//   reserve(C, at)                        its own buffers, each at its place in the order of reservations (ReserveAt)
//   accept(st, ratio)                     what the gate writes into the state of a pair it lets through
//   search(C, phase)                      the move that goes with a search, and C.nn_search
//   iteration(C)                          one iteration of every running pair, up to the kernel that writes the status bytes
//   result(st, D, R)                      the correspondences and the pose of a pair that ran
#pragma once
#include "cloud.h"
#include "refine_dev.h"
#include "refine_plan.h"

namespace rfdev {

// half of the free device memory: what the chunk planners (refine_plan.h) may spend
inline int refine_budget(ghicp_ctx* ctx, size_t* budget) {
  *budget = (size_t)1 << 30;
#ifndef HIPSIM
  size_t free_b = 0, total_b = 0;
  GH_HIP(hipMemGetInfo(&free_b, &total_b));
  *budget = free_b / 2;
#endif
  return GHICP_OK;
}

// Where a method's own buffers come among the chunk's: a fresh context allocates in the order of the reservations, and the loops are timed with
// the buffers at the addresses that order gives them (the select histograms after the partial records, the Mahalanobis matrices among the
// per-point arrays, the reciprocal stage last)
enum ReserveAt { RESERVE_PER_POINT, RESERVE_PER_PAIR, RESERVE_LAST };
enum SearchPhase { SEARCH_FIRST, SEARCH_LOOP, SEARCH_FINAL };  // before the gate and the first iteration / before a later iteration / for the output cloud

template <typename M>
struct RfChunk {
  using Args = typename M::Args;
  using Pair = typename Args::pair_t;
  using State = typename Args::state_t;
  using Result = typename M::Result;
  ghicp_ctx* ctx;
  hipStream_t s;
  M& m;
  const typename M::Params* P;  // use_trimmed, thre_dis, min_overlap: the gate
  const ghicp_cloud* const* S;
  const ghicp_cloud* const* T;
  const double* Rt_init;
  Result* out;
  int b0, np;            // the chunk's pairs: [b0, b0 + np) of the call's
  long long npts;        // source points of the chunk
  int max_gs, running;   // blocks of the largest source (256 points each); pairs still in their loop
  std::vector<Pair> hd;  // host mirrors of the descriptors and states
  std::vector<State> hs;
  std::vector<unsigned> hovl;
  Pair* dd;              // the descriptors on the device (A.pair)
  Args A;

  RfChunk(ghicp_ctx* c, M& method, const typename M::Params* prm, const ghicp_cloud* const* src, const ghicp_cloud* const* tgt, const double* init, Result* o)
      : ctx(c), s(c->stream), m(method), P(prm), S(src), T(tgt), Rt_init(init), out(o) {}

  // ---- the stages in the order they run
  void begin(int first, int count) {  // every pair's descriptor, state and result as a refused pair leaves them
    const float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    b0 = first;
    np = count;
    hd.assign((size_t)np, Pair());
    hs.assign((size_t)np, State());
    npts = 0;
    max_gs = running = 0;
    for (int q = 0; q < np; q++) {
      const ghicp_cloud *a = S[b0 + q], *b = T[b0 + q];
      Result& R = out[b0 + q];
      memset(&R, 0, sizeof(R));
      Pair& D = hd[q];
      memset(&D, 0, sizeof(D));
      for (int e = 0; e < 16; e++) D.init[e] = Rt_init ? (float)Rt_init[(size_t)(b0 + q) * 16 + e] : I16[e];
      State& st = hs[q];
      memset(&st, 0, sizeof(st));
      m.pair(a, b, D, st, R);  // (also for an empty pair: its state must be whole; its own descriptor fields are set and never read, ns = 0)
      D.ns = (int)a->m;
      D.off = npts;
      if (a->m == 0 || b->m == 0) {  // nothing to launch: the answers of ghicp_icp / ghicp_gicp for an empty cloud
        st.refused = 1;
        D.ns = 0;
        float ratio = 1.0f;
        if (P->use_trimmed) {
          ratio = a->m > 0 ? (float)((0.01 + 0) / (double)a->m) : 0.f;
          R.stats.overlap = ratio;
        }
        if (!(P->use_trimmed && ratio < P->min_overlap)) { R.stats.done = 1; R.stats.reason = GHICP_ICP_NO_CORRESPONDENCES; }
        continue;
      }
      D.X.fine = grid_of(b->rf_fine, b->rf_fpts, b->rf_fstart);
      D.X.coarse = grid_of(b->rf_coarse, b->rf_cpts, b->rf_cstart);
      D.tgt = b->ds.as<float4>();
      D.src = a->ds.as<float4>();
      npts += a->m;
      max_gs = max(max_gs, cdiv(a->m, 256));
      running++;
    }
  }

  int reserve() {  // everything the loop touches: nothing allocates inside it
    memset(&A, 0, sizeof(A));
    unsigned* misc;
    GH_TRY(ctx->reserve(B_RF_DESC, (size_t)np, &dd));
    GH_TRY(ctx->reserve(B_ICP_STATE, (size_t)np, &A.st));
    GH_TRY(ctx->reserve(B_ICP_CUR, (size_t)npts + 1, &A.cur));
    GH_TRY(ctx->reserve(B_ICP_NN, (size_t)npts + 1, &A.nn));
    GH_TRY(ctx->reserve(B_ICP_ND, (size_t)npts + 1, &A.nd));
    GH_TRY(m.reserve(*this, RESERVE_PER_POINT));
    GH_TRY(ctx->reserve(B_ICP_PEND, (size_t)npts + 4, &A.pend));
    GH_TRY(ctx->reserve(B_ICP_PART, (size_t)np * icpdev::NBLK * icpdev::NPART, &A.part));
    GH_TRY(m.reserve(*this, RESERVE_PER_PAIR));
    GH_TRY(ctx->reserve(B_RF_MISC, (size_t)np * 3, &misc));
    A.pair = dd;
    A.pendc = misc;
    A.ovl = misc + np;
    A.flag = reinterpret_cast<unsigned char*>(misc + 2 * (size_t)np);
    return m.reserve(*this, RESERVE_LAST);
  }

  int upload_states() { return ctx->upload_table(hs.data(), (size_t)np * sizeof(State), A.st); }
  int upload() {
    GH_TRY(ctx->upload_table(hd.data(), (size_t)np * sizeof(Pair), dd));
    return upload_states();
  }

  // the 1-NN of every point of cur in its pair's target.  `moved`: what the method launches between the counters' reset and the search -- GICP's
  // apply follows the memset, ICP's transform precedes it (IcpMethod::search launches it before it calls this): each loop keeps its sequence
  template <typename F>
  int nn_search(int final, F moved) {
    GH_HIP(hipMemsetAsync(A.pendc, 0, (size_t)np * sizeof(unsigned), s));
    moved();
    hipLaunchKernelGGL(k_chunk_nn_fine<Args>, dim3(max_gs, np), dim3(256), 0, s, A, final);
    hipLaunchKernelGGL(k_chunk_nn_coarse<Args>, dim3(min(cdiv(max_gs * 256ll, 4), COARSE_BLK), np), dim3(256), 0, s, A, final);
    GH_HIP(hipGetLastError());
    return GHICP_OK;
  }
  int nn_search(int final) { return nn_search(final, [] {}); }

  // calOverlap from the first search (common_reg.cpp:64-74, 240-246); a host wait.  No kernel has written a state yet
  int gate() {
    if (!P->use_trimmed) return GHICP_OK;
    GH_HIP(hipMemsetAsync(A.ovl, 0, (size_t)np * sizeof(unsigned), s));
    hipLaunchKernelGGL(k_chunk_overlap<Args>, dim3(max_gs, np), dim3(256), 0, s, A, P->thre_dis * P->thre_dis);
    hovl.assign((size_t)np, 0u);
    GH_HIP(hipMemcpyAsync(hovl.data(), A.ovl, (size_t)np * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    GH_HIP(hipStreamSynchronize(s));
    running = 0;
    for (int q = 0; q < np; q++) {
      State& st = hs[q];
      if (st.refused) continue;
      const float ratio = (float)((0.01 + (int)hovl[q]) / (double)hd[q].ns);  // common_reg.cpp:313
      out[b0 + q].stats.overlap = ratio;
      if (ratio < P->min_overlap) { st.refused = 1; continue; }  // "This registration would not be done"
      m.accept(st, ratio);
      running++;
    }
    return upload_states();
  }

  int status() {  // one byte per pair on the pinned record; a host wait
    static_assert(kRefineMaxChunk <= 4096, "one status byte per pair must fit the pinned scratch");
    unsigned char* pin = reinterpret_cast<unsigned char*>(ctx->pinned);
    GH_HIP(hipGetLastError());
    GH_HIP(hipMemcpyAsync(pin, A.flag, (size_t)np, hipMemcpyDeviceToHost, s));
    GH_HIP(hipStreamSynchronize(s));
    running = 0;
    for (int q = 0; q < np; q++) running += pin[q] ? 0 : 1;
    return GHICP_OK;
  }

  // output = the final transformation * input, then getFitnessScore() on it; the states come back (`kt`: the chunk's stage timer)
  int finish(hipEvent_t kt) {
    GH_TRY(m.search(*this, SEARCH_FINAL));
    hipLaunchKernelGGL(k_chunk_sum<Args>, dim3(icpdev::NBLK, np), dim3(256), 0, s, A);
    hipLaunchKernelGGL(k_chunk_fitness<Args>, dim3(cdiv(np, 64)), dim3(64), 0, s, A, np);
    GH_HIP(hipGetLastError());
    GH_HIP(hipMemcpyAsync(hs.data(), A.st, (size_t)np * sizeof(State), hipMemcpyDeviceToHost, s));
    ctx->kt_end(M::TIMER, kt);
    GH_HIP(hipStreamSynchronize(s));
    for (int q = 0; q < np; q++) {
      const State& st = hs[q];
      if (st.refused) continue;  // refused (or empty): as begin() left it
      Result& R = out[b0 + q];
      R.stats.done = 1;
      R.stats.iterations = st.iterations;
      R.stats.converged = st.converged;
      R.stats.reason = st.reason;
      R.stats.mse = st.mse;
      R.stats.fitness = st.fit_sum / (double)hd[q].ns;
      m.result(st, hd[q], R);
    }
    return GHICP_OK;
  }

  // every chunk of the planner's bounds, one after the other
  int run(const std::vector<int>& bounds) {
    for (size_t ch = 0; ch + 1 < bounds.size(); ch++) {
      begin(bounds[ch], bounds[ch + 1] - bounds[ch]);
      if (running == 0) continue;
      GH_TRY(reserve());
      hipEvent_t kt = ctx->kt_begin(M::TIMER);
      GH_TRY(upload());
      // the first search serves the overlap gate and the first iteration: both see the source under its initial pose
      GH_TRY(m.search(*this, SEARCH_FIRST));
      GH_TRY(gate());
      for (bool have_nn = true; running > 0; have_nn = false) {
        if (!have_nn) GH_TRY(m.search(*this, SEARCH_LOOP));
        GH_TRY(m.iteration(*this));
        GH_TRY(status());
      }
      GH_TRY(finish(kt));
    }
    return GHICP_OK;
  }

  static icpdev::NnGrid grid_of(const GridDesc& d, const DevBuf& pts, const DevBuf& start) {
    return icpdev::NnGrid{d, pts.as<float4>(), start.as<unsigned>(), 1.0f / d.inv};
  }
};

}  // namespace rfdev
