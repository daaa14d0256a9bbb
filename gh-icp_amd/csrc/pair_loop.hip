// The persistent pair loop of the GH-ICP iteration (loop.hip hands it the Kuhn-Munkres batches whose graphs fit the LDS-resident solver): the
// stages of loop_dev.h as out-of-line calls, the kernel k_pair_loop, and its launch per LDS-occupancy class with CU confinement (run_pair_loop).
#include "loop_dev.h"
#include "km4_dev.h"

namespace {

// One 256-thread workgroup = one SOLVE SLOT: it pops a pair from the class
// queue and runs that pair's whole GH-ICP loop (ghicp_reg.cpp:49-103: calED + calCD_* sweep, penalty, graph build, Kuhn-Munkres
// solve, transformestimation, adjustweight, iterate until converged), then pops the next pair.  No kernel boundary, no host poll
// and no other pair stands between two iterations of a pair, so a slot is never idle while its queue holds work: converged pairs
// free their slot at once and the next pair is admitted at once (continuous batching at pair granularity; per pair the order of
// ghicp_reg.cpp:49-103 is kept).  The stages are the SAME device functions the stand-alone kernels run, called for every block
// coordinate in turn.  (The sweep's column chunks are sized per path -- one workgroup sweeps a pair here, many workgroups a batch in the
// per-stage path -- so the f64 sums CDmean / CDstd may differ in the last bits between the two paths: N6 of DESIGN.md §2; everything
// that is compared bit for bit -- matches, solver, rigid solve -- is the same code on the same values.)  Stage scratch (13 KB) overlays
// the solver's LDS.
constexpr int PL_SCRATCH = (CHUNK_MAX * 3 + 16 + 32) * 8 + 20 * 4;

// The stages as out-of-line calls: the persistent kernel's register budget is then the LARGEST stage's, not what the register
// allocator makes of all of them inlined into one loop (256 VGPRs + scratch, one workgroup per CU, when everything is inlined).
template <int FT>
__device__ __noinline__ void pl_sweep(const LoopProb& P, double* sB, double* red) {
  const int rbA = cdiv_dev(P.C.ks > 0 ? P.C.ks : 1, ROWS);
  for (int by = 0; by < P.C.nchunk_b; by++)
    for (int bx = 0; bx < rbA; bx++) {
      __syncthreads();
      dev_cd_rowmin<FT, false>(P, bx, by, sB, red);
    }
  __syncthreads();
  dev_penalty(P, red);
  __syncthreads();
}
template <int FT>
__device__ __noinline__ void pl_graph(const LoopProb& P, int* ired) {
  const int rb4 = cdiv_dev(P.C.n, 4);
  for (int bx = 0; bx < rb4; bx++) dev_km_csr<FT, 0>(P, bx);
  __syncthreads();
  dev_km_scan_desc(P, ired);
  __syncthreads();
  for (int bx = 0; bx < rb4; bx++) dev_km_csr<FT, 1>(P, bx);
  __syncthreads();
}
// ---- The persistent loop's own stages for the Kuhn-Munkres path (GHICP_LOOP_FUSE, default on; DESIGN.md §6 "One combined-distance pass").
// pl_sweep / pl_graph above evaluate CD(i, j) three times per iteration for all K_S x K_T pairs (sums, count, fill) and keep a row arg-min
// that only NN / NNR read.  Here: ONE pass takes the sums -- same block coordinates, same thread per row, same pivot, same order of the
// additions, same gh_block_sum into the same psum slots, so CDmean, CDstd and the penalty keep their bits -- and, from iteration 2 on, when
// the penalty follows from the previous iteration's state alone (gh_penalty_from_state), decides cd < penalty on the way: per row the count
// and max(-cd) (order free, hence exact) and one bit per (i, j) in a row bitmask.  The fill reads the mask: wave-uniform words, no compare,
// no ballot, 64-column blocks without a member skipped unread; CD is evaluated for the value by the same CdEval as everywhere (loop_dev.h).
// Iterations 0 and 1 and the feature NONE need the sweep's mean first: there the count pass runs as before and writes the mask as well.
// Mask: 32-bit words, word w of row i at mask[w * ks + i] (the sweep's lanes are consecutive rows: coalesced stores), 2 ceil(kt / 64) words
// per row so that the fill reads whole 64-column blocks; all of them are written in every iteration (nothing of an earlier pair is read).
// kpT is staged in LDS once per iteration, behind the stage scratch, when the slot's LDS holds it (else chunk by chunk, as pl_sweep does).
constexpr int PL_KPT_OFF = (PL_SCRATCH + 15) & ~15;

template <int FT, bool MEMB>
__device__ __noinline__ void pl_sweep_km(const LoopProb& P, double* sB, double* red, double* sT, unsigned* mask) {
  typedef typename CdEval<FT>::fd_t fd_t;
  const LoopConst& C = P.C;
  const int ks = C.ks, kt = C.kt, chunk = C.chunk_b, nchunk = C.nchunk_b;
  const int rbA = cdiv_dev(ks > 0 ? ks : 1, ROWS);
  const int it = P.st->it;
  const CdEval<FT> E(P, it);
  const fd_t* F = E.typed(P.FDt);
  const double piv = E.pivot(P);
  const double pen = MEMB ? gh_penalty_from_state(P.st, C, P.wfd, it) : 0.0;
  const int nw32 = 2 * cdiv_dev(kt, 64);
  if (sT) {  // (the slot's LDS is the solver's between two iterations: staged again every time)
    __syncthreads();
    for (int t = threadIdx.x; t < kt * 3; t += ROWS) sT[t] = P.kpT[t];
    __syncthreads();
  }
  for (int by = 0; by < nchunk; by++) {
    const int jb = by * chunk;
    const int je = min(kt, jb + chunk);
    if (sT == nullptr) {
      __syncthreads();
      for (int t = threadIdx.x; t < (je - jb) * 3; t += ROWS) sB[t] = P.kpT[(size_t)jb * 3 + t];
      __syncthreads();
    }
    const double* tB = sT ? sT + (size_t)jb * 3 : sB;
    const int jw = (MEMB && by == nchunk - 1) ? nw32 * 32 : je;  // the last chunk also writes the words beyond kt (no member)
    for (int bx = 0; bx < rbA; bx++) {
      const int a = bx * ROWS + threadIdx.x;
      double s = 0, s2 = 0;
      if (a < ks) {
        const double ax = P.kpS[(size_t)a * 3], ay = P.kpS[(size_t)a * 3 + 1], az = P.kpS[(size_t)a * 3 + 2];
        unsigned cnt = 0;
        double mx = -pen;
        if (MEMB && by > 0) { cnt = P.km_cnt[a]; mx = P.km_lx[a]; }  // this thread's own stores of the chunk before
        for (int j0 = jb; j0 < jw; j0 += 32) {
          unsigned bits = 0;
          if (j0 + 32 <= je) {
            // a full word: the feature distances of 4 columns in flight per wait, then 4 evaluations in the order of the columns (8: spills)
            for (int u0 = 0; u0 < 32; u0 += 4) {
              fd_t f[4];
              if (FT != GHICP_FEATURE_NONE) {
#pragma unroll
                for (int k = 0; k < 4; k++) f[k] = F[(size_t)(j0 + u0 + k) * ks + a];
              }
#pragma unroll
              for (int k = 0; k < 4; k++) {
                const int jj = j0 + u0 + k - jb;
                const double cd = E.cd(E.ed(ax, ay, az, tB[jj * 3], tB[jj * 3 + 1], tB[jj * 3 + 2]), FT != GHICP_FEATURE_NONE ? f[k] : (fd_t)0);
                const double c0 = cd - piv;
                s += c0;
                s2 += c0 * c0;
                if (MEMB && cd < pen) { bits |= 1u << (u0 + k); cnt++; mx = fmax(mx, -cd); }
              }
            }
          } else {
            for (int j = j0; j < je; j++) {
              const int jj = j - jb;
              const double cd = E.cd(E.ed(ax, ay, az, tB[jj * 3], tB[jj * 3 + 1], tB[jj * 3 + 2]), E.at(F, (size_t)j * ks + a));
              const double c0 = cd - piv;
              s += c0;
              s2 += c0 * c0;
              if (MEMB && cd < pen) { bits |= 1u << (j - j0); cnt++; mx = fmax(mx, -cd); }
            }
          }
          if (MEMB) mask[(size_t)(j0 >> 5) * ks + a] = bits;
        }
        if (MEMB) { P.km_cnt[a] = cnt; P.km_lx[a] = mx; }
      }
      const double bs = gh_block_sum(s, red);
      const double bs2 = gh_block_sum(s2, red);
      if (threadIdx.x == 0) {
        const size_t b = (size_t)by * rbA + bx;
        P.psum[b * 2] = bs;
        P.psum[b * 2 + 1] = bs2;
      }
    }
  }
  if (MEMB)
    for (int i = ks + threadIdx.x; i < C.n; i += ROWS) { P.km_cnt[i] = 0u; P.km_lx[i] = -pen; }  // padding rows: all background
  __syncthreads();
  dev_penalty(P, red);
  __syncthreads();
}

// rows wave, wave + 4, ... (what pl_graph gives the same wave): the count pass of iterations 0 and 1 (and of NONE), ballots into the mask; scan; fill
template <int FT, bool MEMB>
__device__ __noinline__ void pl_graph_km(const LoopProb& P, int* ired, const double* sT, unsigned* mask) {
  const int wave = threadIdx.x >> 6;
  const double* tB = sT ? sT : P.kpT;
  if (!MEMB) {
    const CdEval<FT> E(P, P.st->it);
    const double pen = P.st->penalty;
    for (int i = wave; i < P.C.n; i += 4) dev_km_row_count<FT, true>(P, E, tB, pen, i, mask);
  }
  __syncthreads();
  dev_km_scan_desc(P, ired);
  __syncthreads();
  const CdEval<FT> E(P, P.st->it);
  for (int i = wave; i < P.C.ks; i += 4) dev_km_row_fill<FT, true>(P, E, tB, 0.0, i, mask);
  __syncthreads();
}
template <bool PROF>
__device__ __noinline__ void pl_km(const Km2Problem* desc, int km_flags, char* smem, int lds_bytes) {
  const Km2Problem KP = *desc;
  k4_solve_block<PROF, false>(KP, km_flags, smem, lds_bytes, nullptr, (k4_gu16) nullptr);
  __syncthreads();
}
// the compact layout (graphs whose standard layout does not fit the slot's LDS: n = 925..1131 at four slots per CU), a call of its own so
// that the 89 % of the pairs below run the code they always ran
template <bool PROF>
__device__ __noinline__ void pl_km_compact(const Km2Problem* desc, int km_flags, char* smem, int lds_bytes, k4_gu16 scr) {
  const Km2Problem KP = *desc;
  k4_solve_block<PROF, true>(KP, km_flags, smem, lds_bytes, nullptr, scr);
  __syncthreads();
}
template <int FT>
__device__ __noinline__ void pl_solve(const LoopProb& P, double* red, int* ired, double* sh) {
  dev_solve<FT>(P, red, ired, sh);
  __syncthreads();
}

// The 100 MHz clock as a scalar: the kernel's time sums then live in scalar registers, not in vector registers that have to survive every stage call.
__device__ inline unsigned long long pl_now() {
  const unsigned long long t = __builtin_amdgcn_s_memrealtime();
  return ((unsigned long long)k4_uni((unsigned)(t >> 32)) << 32) | k4_uni((unsigned)t);
}

template <int FT, bool PROF>
__global__ __launch_bounds__(K4_T, 4) void k_pair_loop(const LoopProb* __restrict__ probs, const int* __restrict__ order, const int npairs, int* qhead,
                                                  const int km_flags, const int lds_bytes, unsigned long long* lstat, int* progress,
                                                  const int* __restrict__ order2, const int npairs2, int* qhead2,
                                                  unsigned short* __restrict__ scr, const long long scr_stride,
                                                  unsigned* mask_all, const long long mask_stride) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* sB = reinterpret_cast<double*>(smem);
  double* red = sB + CHUNK_MAX * 3;
  double* sh = red + 16;
  int* ired = reinterpret_cast<int*>(sh + 32);
  volatile int* s_idx = ired + 18;  // (no static LDS in this kernel: the launch may ask for all 160 KB as dynamic LDS)
  const unsigned long long t_slot0 = lstat ? pl_now() : 0ull;
  unsigned long long t_solve = 0ull, t_solve_max = 0ull, n_solve = 0ull, t_sweep = 0ull, t_graph = 0ull, t_tail = 0ull;
  // A slot is one wave's dependent instruction stream for most of its life (the solver's flood and DFS), and in the tail of a batch it
  // shares its SIMD with the throughput kernels of the next batch's front end: behind 7 ALU-bound waves it would get every eighth issue
  // slot.  The heaviest matrices of the 64 bench scenes are the LATE iterations of the slowest pairs -- exactly the tail --, ~240 ms
  // alone by the model (scripts/km_hazard_survey.py; none of 2220 solves takes the hazard fallback), yet default runs show single solves
  // of 1-4 s (pair_loop_stats.longest_solve_ms).  Highest wave priority: the slot wins the arbitration whenever it can issue at all.
  __builtin_amdgcn_s_setprio(3);
  // (round 6) a slot whose own queue is dry goes on with the queue of the class of SMALLER graphs (order2: they fit its LDS): the slots of the
  // confined three-per-CU class used to leave one by one while the class's last pairs finished, and the launch that re-used their CUs for the
  // other class waited behind the whole kernel in stream order -- 110-180 of 924 slots idle for ~2.2 s of a 9.5 s batch
  // (profiles/r06_call10_log.txt: 924 -> 816 -> 744 before the 988 of the re-launch)
  for (int qsel = 0; qsel < 2; qsel++) {
  const int* const ord = qsel == 0 ? order : order2;
  const int np = qsel == 0 ? npairs : npairs2;
  int* const qh = qsel == 0 ? qhead : qhead2;
  if (ord == nullptr) break;
  for (;;) {
    __syncthreads();
    if (threadIdx.x == 0) *s_idx = atomicAdd(qh, 1);
    __syncthreads();
    const int q = k4_uni((int)*s_idx);  // one value for the workgroup: as a scalar, so that P and what is read through it live in scalar registers across the stage calls
    if (q >= np) break;
    const LoopProb& P = probs[ord[q]];
    if (threadIdx.x == 0 && lstat) P.st->t_begin = pl_now();
    unsigned long long t_pair_max = 0ull;
    int it_pair_max = 0;
    while (k4_uni(*(volatile int*)&P.st->done) == 0) {  // (a scalar: what the loop carries -- the time sums -- is then not divergent at its exit)
      // GHICP_LOOP_FUSE (mask_all: this launch's membership masks, one region per slot; nullptr: the three passes of before).  The fused stages
      // need whole mask words per column chunk: one chunk, or chunks of CHUNK_MAX columns -- what pick_chunks gives this path.  kpT is staged
      // behind the stage scratch when the slot's LDS holds it.  (Worked out per iteration: nothing of it lives across the stage calls.)
      unsigned* const mask = mask_all ? mask_all + (size_t)blockIdx.x * (size_t)mask_stride : (unsigned*)nullptr;
      const bool fuse = mask != nullptr && (P.C.nchunk_b == 1 || (P.C.chunk_b & 31) == 0);
      double* const sT = PL_KPT_OFF + (long long)P.C.kt * 24 <= (long long)lds_bytes ? reinterpret_cast<double*>(smem + PL_KPT_OFF) : (double*)nullptr;
      if (lstat) t_sweep -= pl_now();
      // calED + calCD_* + sums + penalty (ghicp_reg.cpp:114-139, 216-341), then the sparse graph of findcorrespondenceKM
      // (ghicp_reg.cpp:348-365): count, scan, fill
      if (!fuse) {
        pl_sweep<FT>(P, sB, red);
        if (lstat) { const unsigned long long x = pl_now(); t_sweep += x; t_graph -= x; }
        pl_graph<FT>(P, ired);
      } else if (FT != GHICP_FEATURE_NONE && k4_uni(*(volatile int*)&P.st->it) > 1) {  // the penalty is known before the sweep: membership inside it
        pl_sweep_km<FT, FT != GHICP_FEATURE_NONE>(P, sB, red, sT, mask);
        if (lstat) { const unsigned long long x = pl_now(); t_sweep += x; t_graph -= x; }
        pl_graph_km<FT, FT != GHICP_FEATURE_NONE>(P, ired, sT, mask);
      } else {
        pl_sweep_km<FT, false>(P, sB, red, sT, mask);
        if (lstat) { const unsigned long long x = pl_now(); t_sweep += x; t_graph -= x; }
        pl_graph_km<FT, false>(P, ired, sT, mask);
      }
      const unsigned long long t0 = lstat ? pl_now() : 0ull;
      // Km::kmsolve (km.cpp:40-126); the layout per pair from its n (scr: this slot's region of the compact layout's global scratch)
      if (k4_takes_compact(P.C.n, km_flags, lds_bytes))
        pl_km_compact<PROF>(P.km_desc, km_flags, smem, lds_bytes, scr ? (k4_gu16)(scr + (size_t)blockIdx.x * (size_t)scr_stride) : (k4_gu16) nullptr);
      else
        pl_km<PROF>(P.km_desc, km_flags, smem, lds_bytes);
      if (lstat) {
        const unsigned long long dt = pl_now() - t0;
        t_graph += t0; t_tail -= t0 + dt;
        t_solve += dt; t_solve_max = dt > t_solve_max ? dt : t_solve_max; n_solve++;
        if (dt > t_pair_max) { t_pair_max = dt; it_pair_max = k4_uni(*(volatile int*)&P.st->it); }
      }
      pl_solve<FT>(P, red, ired, sh);  // Km::output, transformestimation, adjustweight (ghicp_reg.cpp:416-460, 605-927)
      if (lstat) t_tail += pl_now();
    }
    if (threadIdx.x == 0 && lstat) {
      P.st->t_end = pl_now();
      P.st->t_solve_max = t_pair_max;
      P.st->it_solve_max = it_pair_max;
      // HW_ID (hwreg 4): CU_ID [11:8], SH_ID [12], SE_ID [15:13]; XCC_ID (hwreg 20): [3:0]
      P.st->hw_id = ((unsigned)__builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11)) & 0xFFFFu) | (((unsigned)__builtin_amdgcn_s_getreg((20) | (0 << 6) | (3 << 11)) & 0xFu) << 16);
    }
    if (threadIdx.x == 0 && progress) __hip_atomic_fetch_add(progress, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  }
  if (threadIdx.x == 0 && lstat) {  // launch record: first slot start, last slot end, sum / max of the solve times, solves, sum of slot lifetimes
    const unsigned long long t1 = pl_now();
    atomicMax(&lstat[0], (1ull << 62) - t_slot0);
    atomicMax(&lstat[1], t1);
    atomicAdd(&lstat[2], t_solve);
    atomicMax(&lstat[3], t_solve_max);
    atomicAdd(&lstat[4], n_solve);
    atomicAdd(&lstat[5], t1 - t_slot0);
    atomicAdd(&lstat[6], 1ull);
    atomicAdd(&lstat[8], t_sweep);  // the stages around the solve, summed over all pair-iterations of the batch (ghicp_ctx_pair_loop_stats)
    atomicAdd(&lstat[9], t_graph);
    atomicAdd(&lstat[10], t_tail);
  }
}

// Launches the persistent pair loop: one launch per LDS-occupancy class of the batch (gh_km4_plan: problems per CU, largest graphs
// first), all classes concurrently -- class 0 on the context's stream, the others on auxiliary streams forked from and joined into
// it -- each with its own queue head.  A launch has at most (slots per CU x CUs) workgroups; every workgroup pops pairs until its
// queue is empty.  Returns when every pair of the batch has converged (or hit max_iter).
// (Error path, round-3 advisor: class launches that are already running write the batch's states; whoever returns early waits for
// every stream first -- gh_join_aux -- so that the caller may reuse the context's buffers.  Auxiliary streams inherit the context's CU
// mask (ghicp_ctx_set_cu_mask); a masked stream handed in through ghicp_ctx_set_stream is not inspected: documented in ghicp_c.h.)
static void gh_join_aux(ghicp_ctx* ctx) {
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->confine_stream) (void)hipStreamSynchronize(ctx->confine_stream);
  if (ctx->rest_stream) (void)hipStreamSynchronize(ctx->rest_stream);
  for (hipStream_t a : ctx->aux_streams) (void)hipStreamSynchronize(a);
}
#define GH_HIP_JOIN(call)                                                                                     \
  do {                                                                                                        \
    const hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess) { gh_join_aux(ctx); return ctx->fail(GHICP_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); } \
  } while (0)
// ---- Two classes, three and four slots per CU: the three-per-CU class on its own CUs (see ghicp_ctx::loop_confine).  Their number follows
// the class's share w of the batch's work: 3 B slots of 3 B + 4 (CUs - B) should do w of it, with a margin of 15 % on the caller's prior (iterations x n^2 in bench.py: measured, call 6 -- 392.9 -> 421.5 pairs/s on one box; the prior iterations x n with 10-20 % margin, calls 7 and 8, gave the class fewer CUs and the batch a longer span: 375-384) (its queue must not
// outlast the other one: the four-per-CU slots may use every CU, the confined ones only theirs), spread evenly over the mask's bits.
// Returns B, the CUs of the three-per-CU class, with ctx->confine_stream / rest_stream the masked stream pair for it; 0: the batch runs unconfined.
static int gh_confine_streams(ghicp_ctx* ctx, const Km4Plan& plan) {
  const int nc = plan.nclass;
  int confine_b = 0;
  if (ctx->loop_confine && nc == 2 && plan.per_cu[0] == 3 && plan.per_cu[1] == 4 && plan.count[0] > 0 && plan.count[1] > 0 && ctx->cu_mask.empty() &&
      ctx->num_cu >= 8 && ctx->num_cu <= 2048 && plan.weight[0] > 0 && plan.weight[1] > 0) {
    const double w = std::min(0.9, ctx->loop_confine_margin * plan.weight[0] / (plan.weight[0] + plan.weight[1]));
    int B = (int)std::ceil(w * 4.0 * ctx->num_cu / (3.0 + w));
    B = std::max(B, (plan.count[0] >= 3 ? 1 : 0));
    B = std::min(B, std::min(ctx->num_cu / 2, cdiv(plan.count[0], 3)));
    if (B >= 1) {
      if (ctx->confine_stream == nullptr || ctx->rest_stream == nullptr || ctx->confine_cus != B) {
        // B follows the caller's cost prior from batch to batch: the masked stream pairs are kept per B (a handful of values in practice)
        // instead of being destroyed and re-created -- with a stream synchronisation -- on the launch path (round-5 advisor)
        ctx->confine_stream = ctx->rest_stream = nullptr;
        ctx->confine_cus = 0;
        for (auto& e : ctx->confine_cache)
          if (e.cus == B) { ctx->confine_stream = e.confined; ctx->rest_stream = e.rest; ctx->confine_cus = B; }
        if (ctx->confine_cus != B) {
          if (ctx->confine_cache.size() >= 16) {  // bounded: drop them all (nothing of this context runs on them between two batches)
            for (auto& e : ctx->confine_cache) {
              (void)hipStreamSynchronize(e.confined); (void)hipStreamDestroy(e.confined);
              (void)hipStreamSynchronize(e.rest); (void)hipStreamDestroy(e.rest);
            }
            ctx->confine_cache.clear();
          }
          std::vector<uint32_t> mask((size_t)cdiv(ctx->num_cu, 32), 0u), rest((size_t)cdiv(ctx->num_cu, 32), 0u);
          for (int i = 0; i < ctx->num_cu; i++) {
            const bool in = (long long)(i + 1) * B / ctx->num_cu > (long long)i * B / ctx->num_cu;
            (in ? mask : rest)[(size_t)i >> 5] |= 1u << (i & 31);
          }
          hipStream_t sa = nullptr, sb = nullptr;
          if (hipExtStreamCreateWithCUMask(&sa, (uint32_t)mask.size(), mask.data()) == hipSuccess &&
              hipExtStreamCreateWithCUMask(&sb, (uint32_t)rest.size(), rest.data()) == hipSuccess) {
            ctx->confine_cache.push_back({B, sa, sb});
            ctx->confine_stream = sa; ctx->rest_stream = sb; ctx->confine_cus = B;
          } else {  // no masked streams on this runtime: the batch runs unconfined; the runtime's sticky error must not fail the launch below
            if (sa) (void)hipStreamDestroy(sa);
            if (sb) (void)hipStreamDestroy(sb);
            (void)hipGetLastError();
          }
        }
      }
      if (ctx->confine_cus == B) confine_b = B;
    }
  }
  return confine_b;
}

}  // namespace

template <int FT>
int run_pair_loop(ghicp_ctx* ctx, const LoopProb* dprobs, int nb, const Km4Plan& plan, int* dqheads) {
  hipStream_t s = ctx->stream;
  const int nc = plan.nclass;
  if (nc <= 0) return GHICP_OK;
  while ((int)ctx->aux_streams.size() < nc - 1) {
    hipStream_t a = nullptr;
    if (ctx->cu_mask.empty()) GH_HIP(hipStreamCreateWithFlags(&a, hipStreamNonBlocking));
    else GH_HIP(hipExtStreamCreateWithCUMask(&a, (uint32_t)ctx->cu_mask.size(), ctx->cu_mask.data()));  // stay on the context's compute units
    ctx->aux_streams.push_back(a);
  }
  while ((int)ctx->aux_events.size() < nc + 2) {
    hipEvent_t e = nullptr;
    GH_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ctx->aux_events.push_back(e);
  }
  if (!ctx->progress_host) {
    if (hipHostMalloc((void**)&ctx->progress_host, 64, hipHostMallocMapped) != hipSuccess)
      return ctx->fail(GHICP_ERR_HIP, "pair loop: mapped progress counter allocation failed");
  }
  *(volatile int*)ctx->progress_host = 0;
  ctx->progress_live.store(true, std::memory_order_release);
  const bool prof = ctx->km_stats;
  const auto kern = prof ? &k_pair_loop<FT, true> : &k_pair_loop<FT, false>;
  const void* fn = reinterpret_cast<const void*>(kern);
  GH_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  const int kflags = ctx->km_kflags();  // test hooks: one phase through the hazard fallback; the compact layout forced
  const auto lds_of = [&](int c) { return std::max(std::max(plan.lds[c], (size_t)PL_SCRATCH + 64), (size_t)ctx->loop_min_lds); };  // a slot's LDS
  // Per solve slot one region of global scratch for the compact Kuhn-Munkres layout (only when a graph can take that layout) and one of the
  // fused stages' membership mask (GHICP_LOOP_FUSE: 2 ceil(n / 64) words of 32 bits per row) -- sized by slots, not by pairs, and a range of
  // its own for every launch of the batch (a class is launched twice when its queue is also served from the confined CUs)
  int n_all = 1;
  size_t regions = 0;
  bool compact = ctx->km_compact_from > 0;
  for (int c = 0; c < nc; c++) {
    n_all = std::max(n_all, plan.nmax[c]);
    regions += 2 * (size_t)std::min(plan.count[c], 4 * ctx->num_cu);
    compact = compact || k4_lds_need(plan.nmax[c], false) > (long long)lds_of(c);
  }
  unsigned short* scr = nullptr;
  unsigned* msk = nullptr;
  const long long scr_stride = compact ? k4_scratch_u16(n_all) : 0, msk_stride = ctx->loop_fuse ? 2ll * cdiv(n_all, 64) * n_all : 0;
  if (compact) GH_TRY(ctx->reserve(B_KM_SLACK, regions * (size_t)scr_stride, &scr));
  if (ctx->loop_fuse) GH_TRY(ctx->reserve(B_KM_MASK, regions * (size_t)msk_stride, &msk));
  size_t scr_next = 0;  // regions handed out
  GH_HIP(hipMemsetAsync(dqheads, 0, 16 * sizeof(int), s));
  // one launch record per BATCH: the classes of a batch share it (first slot start, last slot end, sums over all slots), and the batch's
  // capacity is what can be resident at once: all its workgroups, but not more than the slots of the roomiest class (the classes compete
  // for the same CUs)
  unsigned long long* lstat = nullptr;
  int batch_slots = 0, batch_grid = 0;
  if (ctx->kt_on && ctx->km_launches < ghicp_ctx::KM_LSTAT_MAX) {
    GH_TRY(ctx->reserve(B_KM_LSTAT, (size_t)ghicp_ctx::KM_LSTAT_MAX * ghicp_ctx::KM_LSTAT_W, &lstat));
    lstat += ctx->km_launches * ghicp_ctx::KM_LSTAT_W;
  }
  const int confine_b = gh_confine_streams(ctx, plan);
  // the one launch: `grid` slots for class c's queue on stream sc, each with the next region of scratch and mask; steal: then class 1's queue
  const auto launch = [&](hipStream_t sc, int grid, int c, bool steal) {
    const size_t lds = lds_of(c);
    unsigned short* scr_c = scr ? scr + scr_next * (size_t)scr_stride : nullptr;
    unsigned* msk_c = msk ? msk + scr_next * (size_t)msk_stride : nullptr;
    scr_next += (size_t)grid;
    hipEvent_t kd = ctx->kt_begin_on(KT_PAIR_LOOP_DISPATCH, sc);  // this dispatch alone, on its own stream (behind the fork event)
    hipLaunchKernelGGL(kern, dim3(grid), dim3(K4_T), lds, sc, dprobs, (const int*)(plan.d_order + plan.begin[c]), plan.count[c], dqheads + c, kflags,
                       (int)lds, lstat, ctx->progress_host, steal ? (const int*)(plan.d_order + plan.begin[1]) : (const int*)nullptr,
                       steal ? plan.count[1] : 0, steal ? dqheads + 1 : (int*)nullptr, scr_c, scr_stride, msk_c, msk_stride);
    ctx->kt_end_on(KT_PAIR_LOOP_DISPATCH, kd, sc);
  };
  hipEvent_t kt = ctx->kt_begin(KT_PAIR_LOOP);
  GH_HIP_JOIN(hipEventRecord(ctx->aux_events[0], s));
  bool stole = false;
  for (int c = 0; c < nc; c++) {
    if (plan.count[c] <= 0) continue;
    // confined: the three-per-CU class on its CUs; the four-per-CU class on all the OTHER CUs (if it could use every CU, its slots would
    // take the confined class's CUs first and never leave) and, behind the confined class in stream order, on those CUs as well -- the
    // same queue, so the late slots help drain it
    const bool confined = confine_b > 0;
    hipStream_t sc = confined ? (c == 0 ? ctx->confine_stream : ctx->rest_stream) : (c == 0 ? s : ctx->aux_streams[(size_t)c - 1]);
    if (c > 0 || confined) GH_HIP_JOIN(hipStreamWaitEvent(sc, ctx->aux_events[0], 0));
    const size_t lds = lds_of(c);
    int per_cu = 0;
    GH_HIP_JOIN(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, K4_T, lds));
    if (per_cu <= 0) gh_join_aux(ctx);
    if (per_cu <= 0) return ctx->fail(GHICP_ERR_INTERNAL, "pair loop: a workgroup with %zu bytes of LDS does not fit a CU", lds);
    const int slots = per_cu * (confined ? (c == 0 ? confine_b : ctx->num_cu - confine_b) : ctx->num_cu);
    int grid = std::min(plan.count[c], slots);
    if (ctx->loop_slots_cap > 0) grid = std::min(grid, ctx->loop_slots_cap);  // test hook (GHICP_LOOP_SLOTS)
    // capacity of the batch = the most slots the chip can hold at once: the roomiest class on EVERY CU.  (Round 5 added up the confined
    // classes' shares, 3 B + 4 (CUs - B); but once the three-per-CU class has drained, its CUs take four slots of the other class, so the
    // slot lifetimes of a batch could exceed that "capacity" x span: idle_slot_fraction -0.14 in profiles/r05_bench_confine1.json --
    // round-5 verdict, weak #5.  Against this bound the LDS the three-per-CU slots leave unused counts as idle, which it is.)
    batch_slots = std::max(batch_slots, per_cu * ctx->num_cu);
    batch_grid += grid;
    // the confined class's slots go on with the other class's queue when their own is dry (smaller graphs: they fit)
    const bool steal = confined && c == 0 && plan.lds[1] <= lds;
    stole = stole || steal;
    launch(sc, grid, c, steal);
    GH_HIP_JOIN(hipGetLastError());
    if (c > 0 || confined) {
      GH_HIP_JOIN(hipEventRecord(ctx->aux_events[(size_t)c + 1], sc));
      GH_HIP_JOIN(hipStreamWaitEvent(s, ctx->aux_events[(size_t)c + 1], 0));
    }
    if (confined && c == 1 && !stole) {  // ... and the four-per-CU class once more, on the confined CUs, after the three-per-CU class (only when that class's slots could not take the queue over themselves)
      const int grid2 = std::min(plan.count[c], per_cu * confine_b);
      launch(ctx->confine_stream, grid2, c, false);
      GH_HIP_JOIN(hipGetLastError());
      batch_grid += grid2;
      GH_HIP_JOIN(hipEventRecord(ctx->aux_events[(size_t)nc + 1], ctx->confine_stream));
      GH_HIP_JOIN(hipStreamWaitEvent(s, ctx->aux_events[(size_t)nc + 1], 0));
    }
  }
  ctx->kt_end(KT_PAIR_LOOP, kt);
  if (lstat) {
    ctx->km_slots.push_back(std::min(batch_slots, batch_grid));
    ctx->km_launches++;
  }
  GH_HIP_JOIN(hipStreamSynchronize(s));
  return GHICP_OK;
}
#undef GH_HIP_JOIN

template int run_pair_loop<GHICP_FEATURE_NONE>(ghicp_ctx*, const LoopProb*, int, const Km4Plan&, int*);
template int run_pair_loop<GHICP_FEATURE_BSC>(ghicp_ctx*, const LoopProb*, int, const Km4Plan&, int*);
template int run_pair_loop<GHICP_FEATURE_FPFH>(ghicp_ctx*, const LoopProb*, int, const Km4Plan&, int*);
