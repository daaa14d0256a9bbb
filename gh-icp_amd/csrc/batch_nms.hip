// Round-based non-maximum suppression of the batched front end (FbRun::nms, between the prune and output stages of batch.hip): the decision-round
// kernels k_fb_nmsr_* over the candidates of every cloud of a batch, and their launch sequence.
#include "batch_dev.h"
#include "prims.h"

namespace {

// Greedy non-maximum suppression (keypoint_detect.hpp:149-191) = the lexicographically first maximal independent set of the graph
// "candidates closer than R", taken in rank order (curvature descending, ties: lower point index).  It is the unique fixed point of
//     selected(i)   <=>  every neighbour of higher rank is suppressed
//     suppressed(i) <=>  some neighbour of higher rank is selected                                              
// and both facts are FINAL once established, so they may be established in any order by any number of threads: a candidate decides as
// soon as its higher-ranked neighbours have.  One thread per candidate, every cloud of the batch in the same launches, a handful of
// rounds (the longest chain of decisions a scan needs: 6-11 with synchronous rounds, fewer here because a round sees the decisions
// of the waves that ran before it).  Rounds 2-5 walked the rank-ordered candidates of a cloud with ONE workgroup (nms_dev.h, still the
// single-cloud path): 1.6-2.5 ms per launch with 224 CUs idle -- round-5 verdict, weak #6 / item 7.
//   * candidates are bucketed by cell (side R * 1.0001, the cloud's own grid over the box of its down-sampled points) by a counting
//     sort: histogram, hand-written scan (prims.hip), scatter -- the order inside a cell does not matter, every test is order free;
//   * "suppressed" is decided against per-cell lists of the SELECTED candidates (1-3 entries around a point); "selected" by ONE walk over
//     the neighbouring cells, spread over the rounds: the walk stops at a neighbour of higher rank that is not suppressed and goes on
//     behind it once that neighbour has been suppressed (k_fb_nmsr_round);
//   * the keypoints of a cloud leave in rank order: each selected candidate counts the selected ones of its cloud that outrank it.
// Same set AND order as the greedy sweep (tests/test_gpu_batch.py, test_golden.py: keypoint ids == oracle).
struct NmsrArgs {
  const float4* dsg;          // concatenated down-sampled clouds
  const int* cand;            // candidate -> global point index, ascending
  const double* curv;
  int ctot;
  unsigned* table;            // [0] = 0, [1 + cell]: histogram -> end -> start of the cell's run (see k_fb_nmsr_fill)
  unsigned* ccell;            // candidate -> global cell
  unsigned long long* ckey;   // candidate -> rank key (order-preserving image of the curvature)
  float4* spts;               // slot -> (x, y, z, candidate id); inside a cell the slots are in RANK order (k_fb_nmsr_sort)
  unsigned long long* skey;   // slot -> rank key
  float4* spts0;              // the same two arrays as the scatter left them (cell by cell, arbitrary order inside a cell)
  unsigned long long* skey0;
  unsigned char* state;       // slot -> 0 undecided, 1 selected, 2 suppressed
  int* head;                  // cell -> most recently selected slot, -1: none
  int* next;                  // slot -> next selected slot of its cell
  int* blk;                   // slot -> the neighbour of higher rank this candidate is waiting for (-1: has not looked yet)
  unsigned* upos;             // slot -> where its scan of the neighbouring cells goes on (slot index) ...
  unsigned char* urun;        // ... and in which of the nine runs
  int* sel;                   // per cloud (at coff[b]): the selected slots, in no particular order
  int* kcount;                // per cloud: selected so far
  int* undecided;             // per round: candidates the round left undecided
};

__global__ __launch_bounds__(256) void k_fb_nmsr_keys(const FbBlock* __restrict__ D, NmsrArgs A) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= A.ctot) return;
  const int b = fb_find(D->coff, D->nb, i);
  const GridDesc& g = D->g3[b];
  const int pid = A.cand[i];
  const float4 P = A.dsg[pid];
  const int cx = gh_cell_coord(P.x, g.mn[0], g.inv, g.dim[0]);
  const int cy = gh_cell_coord(P.y, g.mn[1], g.inv, g.dim[1]);
  const int cz = gh_cell_coord(P.z, g.mn[2], g.inv, g.dim[2]);
  const unsigned cell = D->hb[b] + (((unsigned)cx * g.dim[1] + cy) * g.dim[2] + cz);
  A.ccell[i] = cell;
  A.ckey[i] = fb_f64_key(A.curv[pid]);
  atomicAdd(&A.table[1 + cell], 1u);
}

// after the inclusive scan table[1 + c] is the END of cell c's run; every candidate takes the slot below the current end, which leaves
// table[1 + c] = START of cell c = end of cell c - 1: T = table + 1 is then the usual cell table (T[c] .. T[c + 1]), T[ncell] = ctot
__global__ __launch_bounds__(256) void k_fb_nmsr_fill(NmsrArgs A, unsigned ncell) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) A.table[1 + ncell] = (unsigned)A.ctot;
  if (i >= A.ctot) return;
  const unsigned t = atomicSub(&A.table[1 + A.ccell[i]], 1u) - 1u;
  const float4 P = A.dsg[A.cand[i]];
  A.spts0[t] = make_float4(P.x, P.y, P.z, __int_as_float(i));
  A.skey0[t] = A.ckey[i];
}

// Inside a cell the candidates go in RANK order (highest first): every candidate counts the members of its cell that outrank it -- cells
// hold ~10 candidates, a few hundred at most -- and takes that position.  A walk over a cell can then stop at the first entry of lower
// rank, so a candidate near the top of its neighbourhood (the ones that stay undecided longest, and the ones that end up selected)
// looks at a handful of entries per cell instead of all of them (call 6 of round 6: rounds 2-9 were 100-220 us each, held up by the
// few candidates per wave that had to walk their whole neighbourhood, ~200 entries, to find nobody left above them).
__global__ __launch_bounds__(256) void k_fb_nmsr_sort(NmsrArgs A) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= A.ctot) return;
  const float4 P = A.spts0[t];
  const int id = __float_as_int(P.w);
  const unsigned long long key = A.skey0[t];
  const unsigned c = A.ccell[id];
  const unsigned ub = A.table[1 + c], ue = A.table[2 + c];
  unsigned rank = 0;
  for (unsigned u = ub; u < ue; u++) {
    const unsigned long long ku = A.skey0[u];
    rank += (ku > key || (ku == key && __float_as_int(A.spts0[u].w) < id)) ? 1u : 0u;
  }
  const unsigned d = ub + rank;
  A.spts[d] = P;
  A.skey[d] = key;
  A.state[d] = 0;
  A.blk[d] = -1;
  A.next[d] = -1;
  A.urun[d] = 0;
  A.upos[d] = 0u;
}

// One round, for every candidate that has not decided yet:
//   (1) a SELECTED neighbour (per-cell lists of the selected candidates, 1-3 entries around a point) -> suppressed.  A selected neighbour
//       of an undecided candidate always outranks it (nothing is selected next to an undecided candidate of higher rank);
//   (2) otherwise the candidate walks the entries of its nine runs ONCE over all rounds: it stops at the first neighbour of higher rank
//       that is not suppressed and WAITS for it (blk; the position is kept in urun / upos).  The next round looks at that neighbour's
//       state first (one load) and walks on behind it only if it has been suppressed: whatever lies before that position was out of
//       range, of lower rank or suppressed -- all final;
//   (3) the walk reaches the end: every neighbour of higher rank is suppressed -> selected.
// Measured on 32 cfg2 clouds (0.96 M candidates): a full re-scan in every round (call 3) visits 380 M entries, 2.9 ms; the walk without
// step (1) (call 4) needs a round per link of a chain of waiting candidates, hundreds of rounds; with both, a suppression shows one
// round after the selection that causes it and an entry is visited at most once per candidate.
__global__ __launch_bounds__(256) void k_fb_nmsr_round(const FbBlock* __restrict__ D, NmsrArgs A, float r2, int round, int first) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  int waiting = 0;  // no early return: the wave counts its waiting lanes with ONE atomic at the end
  if (t < A.ctot && A.state[t] == 0) {
    const float4 P = A.spts[t];
    const int id = __float_as_int(P.w);
    const int b = fb_find(D->coff, D->nb, id);
    const GridDesc g = D->g3[b];
    const int cx = gh_cell_coord(P.x, g.mn[0], g.inv, g.dim[0]);
    const int cy = gh_cell_coord(P.y, g.mn[1], g.inv, g.dim[1]);
    const int cz = gh_cell_coord(P.z, g.mn[2], g.inv, g.dim[2]);
    int* H = A.head + D->hb[b];
    int verdict = 0;  // 0 go on, 1 wait, 2 suppressed
    if (!first) {     // (1); plain loads: a stale list only postpones the decision by a round.  All 27 list heads are asked for at once
      int hd[27];     // (independent loads: one round trip to L2 instead of 27 dependent ones -- the round is bound by load latency)
#pragma unroll
      for (int r = 0; r < 9; r++) {
        const int x = cx - 1 + r / 3, y = cy - 1 + r % 3;
        const bool in = x >= 0 && x < g.dim[0] && y >= 0 && y < g.dim[1];
        const unsigned base = in ? ((unsigned)x * g.dim[1] + y) * g.dim[2] : 0u;
#pragma unroll
        for (int dz = 0; dz < 3; dz++) {
          const int z = cz - 1 + dz;
          hd[r * 3 + dz] = (in && z >= 0 && z < g.dim[2]) ? H[base + z] : -1;
        }
      }
#pragma unroll
      for (int q = 0; q < 27; q++)
        for (int j = hd[q]; j >= 0 && verdict == 0; j = A.next[j]) {
          const float4 Q = A.spts[j];
          const float dx = Q.x - P.x, dy = Q.y - P.y, dz = Q.z - P.z;
          float d2 = dx * dx;
          d2 += dy * dy;
          d2 += dz * dz;
          if (d2 < r2) verdict = 2;
        }
    }
    if (verdict == 0) {  // (2)
      const int bl = A.blk[t];
      if (bl >= 0) {
        const int sb = A.state[bl];
        verdict = sb == 0 ? 1 : (sb == 1 ? 2 : 0);
      }
    }
    if (verdict == 0) {
      const unsigned long long key = A.skey[t];
      const unsigned* T = A.table + 1 + D->hb[b];
      unsigned tb[9][4];  // the cell table around the candidate: nine columns x (three cells + 1), asked for at once
#pragma unroll
      for (int q = 0; q < 9; q++) {
        const int x = cx - 1 + q / 3, y = cy - 1 + q % 3;
        const bool in = x >= 0 && x < g.dim[0] && y >= 0 && y < g.dim[1];
        const unsigned base = in ? ((unsigned)x * g.dim[1] + y) * g.dim[2] : 0u;
#pragma unroll
        for (int dz = 0; dz < 4; dz++) {
          const int z = cz - 1 + dz;
          tb[q][dz] = (in && z >= 0 && z <= g.dim[2]) ? T[base + z] : 0u;
        }
      }
      const int c_from = A.urun[t];  // cell 0..26 the walk stands in
      const unsigned u_res = A.upos[t];
#pragma unroll
      for (int c = 0; c < 27; c++) {
        if (verdict != 0 || c < c_from) continue;
        const int q = c / 3, dz = c % 3;
        const int z = cz - 1 + dz;
        if (z < 0 || z >= g.dim[2]) continue;
        const unsigned ub = tb[q][dz], ue = tb[q][dz + 1];
        // four entries per step, everything a verdict may need asked for at once (position, rank key, state: independent loads); they
        // are LOOKED AT in slot order = rank order, and the cell is left at the first entry that does not outrank this candidate
        bool below = false;
        for (unsigned u0 = max(ub, c == c_from ? u_res : 0u); u0 < ue && verdict == 0 && !below; u0 += 4u) {
          float4 Q[4];
          unsigned long long K[4];
          int S[4];
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const unsigned u = min(u0 + (unsigned)e, ue - 1u);
            Q[e] = A.spts[u]; K[e] = A.skey[u]; S[e] = A.state[u];
          }
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const unsigned u = u0 + (unsigned)e;
            if (verdict != 0 || below || u >= ue) continue;
            if (!(K[e] > key || (K[e] == key && __float_as_int(Q[e].w) < id))) { below = true; continue; }  // this entry and the rest of the cell rank lower (or it is the candidate itself)
            const float dx = Q[e].x - P.x, dy = Q[e].y - P.y, dz2 = Q[e].z - P.z;
            float d2 = dx * dx;
            d2 += dy * dy;
            d2 += dz2 * dz2;
            if (!(d2 < r2)) continue;
            if (S[e] == 2) continue;
            if (S[e] == 1) { verdict = 2; continue; }
            A.blk[t] = (int)u; A.urun[t] = (unsigned char)c; A.upos[t] = u + 1u;
            verdict = 1;
          }
        }
      }
      if (verdict == 0) {  // (3)
        A.state[t] = 1;
        const int old = atomicExch(&H[((unsigned)cx * g.dim[1] + cy) * g.dim[2] + cz], t);
        A.next[t] = old;
        A.sel[D->coff[b] + atomicAdd(&A.kcount[b], 1)] = t;
      }
    }
    if (verdict == 2) A.state[t] = 2;
    waiting = verdict == 1;
  }
  const unsigned long long wm = __ballot(waiting != 0);
  if ((threadIdx.x & 63) == 0 && wm) atomicAdd(&A.undecided[round], (int)__popcll(wm));
}

// keypoints of cloud b in rank order: position = number of selected candidates of the cloud that outrank this one
__global__ __launch_bounds__(256) void k_fb_nmsr_rank(const FbBlock* __restrict__ D, NmsrArgs A, int* __restrict__ kpg) {
  __shared__ unsigned long long s_key[1024];
  __shared__ int s_id[1024];
  const int b = blockIdx.x;
  const int K = A.kcount[b], c0 = D->coff[b];
  for (int base = blockIdx.y * 256; base < K; base += 256 * gridDim.y) {  // (the trip count is uniform over the workgroup: barriers below)
    const int k = base + threadIdx.x;
    unsigned long long key = 0;
    int id = 0;
    if (k < K) { const int t = A.sel[c0 + k]; key = A.skey[t]; id = __float_as_int(A.spts[t].w); }
    int rank = 0;
    for (int q0 = 0; q0 < K; q0 += 1024) {
      __syncthreads();
      for (int q = threadIdx.x; q < min(1024, K - q0); q += 256) { const int t = A.sel[c0 + q0 + q]; s_key[q] = A.skey[t]; s_id[q] = __float_as_int(A.spts[t].w); }
      __syncthreads();
      const int m = min(1024, K - q0);
      if (k < K)
        for (int q = 0; q < m; q++) rank += (int)(s_key[q] > key) | ((int)(s_key[q] == key) & (int)(s_id[q] < id));
    }
    if (k < K) kpg[c0 + rank] = A.cand[id] - D->moff[b];
  }
}

}  // namespace

// candidate cells (counting sort), decision rounds in sequences of FB_NMS_ROUNDS with a host synchronisation after each, ranks
int FbRun::nms() {
  kpg = nullptr;
  Ktot = 0;
  if (Ctot <= 0) return GHICP_OK;
  NmsrArgs A;
  A.dsg = dsg; A.cand = cand; A.curv = curv; A.ctot = Ctot;
  GH_TRY(ctx->reserve(B_NMSR_TABLE, (size_t)t3 + 4, &A.table));
  GH_TRY(ctx->reserve(B_NMSR_HEAD, (size_t)Ctot + 1, &A.upos));
  GH_TRY(ctx->reserve(B_NMSR_CELL, (size_t)Ctot + 1, &A.ccell));
  GH_TRY(ctx->reserve(B_NMSR_KEY, (size_t)Ctot + 1, &A.ckey));
  GH_TRY(ctx->reserve(B_NMSR_PTS, (size_t)Ctot + 1, &A.spts));
  GH_TRY(ctx->reserve(B_NMSR_SKEY, (size_t)Ctot + 1, &A.skey));
  GH_TRY(ctx->reserve(B_NMSR_PTS0, (size_t)Ctot + 1, &A.spts0));
  GH_TRY(ctx->reserve(B_NMSR_SKEY0, (size_t)Ctot + 1, &A.skey0));
  GH_TRY(ctx->reserve(B_NMSR_STATE, (size_t)Ctot * 2 + 32, &A.state));
  A.urun = A.state + (((size_t)Ctot + 15) & ~(size_t)15);
  GH_TRY(ctx->reserve(B_NMSR_NEXT, (size_t)Ctot * 2 + 2, &A.blk));
  A.next = A.blk + Ctot + 1;
  GH_TRY(ctx->reserve(B_NMSR_LIST, (size_t)t3 + 2, &A.head));
  GH_TRY(ctx->reserve(B_NMSR_SEL, (size_t)Ctot + 1, &A.sel));
  GH_TRY(ctx->reserve(B_FE_KP, (size_t)Ctot + 1, &kpg));
  A.kcount = O->kcount;
  A.undecided = O->nms_und;
  GH_HIP(upload());  // g3 / hb (the device wrote coff itself)
  hipEvent_t kr = ctx->kt_begin(KT_FB_RANK);
  GH_HIP(hipMemsetAsync(A.table, 0, ((size_t)t3 + 2) * sizeof(unsigned), s));
  GH_HIP(hipMemsetAsync(A.head, 0xff, (size_t)t3 * sizeof(int), s));
  GH_HIP(hipMemsetAsync(O->kcount, 0, sizeof(int) * FB_MAX, s));
  hipLaunchKernelGGL(k_fb_nmsr_keys, dim3(cdiv(Ctot, 256)), dim3(256), 0, s, (const FbBlock*)D, A);
  GH_TRY(gh_scan_inclusive_u32(ctx, A.table + 1, (long long)t3));
  hipLaunchKernelGGL(k_fb_nmsr_fill, dim3(cdiv(Ctot, 256)), dim3(256), 0, s, A, (unsigned)t3);
  hipLaunchKernelGGL(k_fb_nmsr_sort, dim3(cdiv(Ctot, 256)), dim3(256), 0, s, A);
  ctx->kt_end(KT_FB_RANK, kr);
  const float r_nms = cfg.reg.radius_nonmax, r2_nms = (float)((double)r_nms * (double)r_nms);
  for (int seq = 0;; seq++) {
    hipEvent_t kn = ctx->kt_begin(KT_NMS_ROUND);
    GH_HIP(hipMemsetAsync(O->nms_und, 0, sizeof(int) * FB_NMS_ROUNDS, s));
    for (int r = 0; r < FB_NMS_ROUNDS; r++)
      hipLaunchKernelGGL(k_fb_nmsr_round, dim3(cdiv(Ctot, 256)), dim3(256), 0, s, (const FbBlock*)D, A, r2_nms, r, (seq == 0 && r == 0) ? 1 : 0);
    ctx->kt_end(KT_NMS_ROUND, kn);
    GH_HIP(hipGetLastError());
    GH_HIP(report());
    if (HO->nms_und[FB_NMS_ROUNDS - 1] == 0) break;  // every candidate has decided
    if (seq > 4096) return ctx->fail(GHICP_ERR_INTERNAL, "ghicp_clouds_recompute: the NMS rounds do not terminate");  // (each sequence decides at least one candidate)
  }
  for (int b = 0; b < nb; b++) {
    clouds[b]->k = HO->kcount[b];
    H->koff[b + 1] = H->koff[b] + HO->kcount[b];
  }
  Ktot = H->koff[nb];
  if (Ktot > 0) {
    hipEvent_t kk = ctx->kt_begin(KT_NMS_ROUND);
    hipLaunchKernelGGL(k_fb_nmsr_rank, dim3(nb, 8), dim3(256), 0, s, (const FbBlock*)D, A, kpg);
    ctx->kt_end(KT_NMS_ROUND, kk);
  }
  return GHICP_OK;
}
