// Batched prepare (gfx950): what ghicp_cloud_prepare_refine / ghicp_cloud_prepare_gicp / ghicp_cloud_prepare_overlap build cloud by cloud --
// the fine + coarse 1-NN grids, the k-NN normals, the GICP covariances, the overlap grid -- for MANY handles in one launch sequence per chunk.
//
// Why: one cloud's preparation is up to six grid builds for the fine cell (a host read per attempt), a coarse and an overlap grid with a
// bounding-box read each, two identical k-NN grids and searches (normals, covariances) and copies out of the context's buffers, all issued
// and waited for per cloud; every recompute invalidates it.  Here the clouds of a chunk are CONCATENATED, as in batch.hip:
//   * boxes: one launch and one host read for the whole list (min / max through the order-preserving int mapping of k_bbox: exact);
//   * a grid kind of all clouds: global cell keys (cell base of the cloud + its own key) -> ONE stable radix sort -> ONE cell table ->
//     k_pp_scatter writes every cloud's run of sorted points (w rebased to the cloud's own index) and its slice of the table (rebased to the
//     cloud's first sorted point) straight into the handle's buffers through a pointer table.  The stable sort keeps a cell's points in
//     down-sampled order, so the bytes are those of gh_grid_build over the cloud alone;
//   * the halving of the fine cell (icp.hip build_index) runs in rounds over the clouds still halving: one build, one count of occupied cells
//     per cloud, ONE host read, the stop rules of build_index per cloud on the host; a cloud that stops has its grid of that round scattered
//     into its handle before the next round overwrites the chunk's buffers;
//   * k-NN: one grid and one k_knn_batch per k; normals and covariances (the kernels of the single-cloud calls) run over the same lists when
//     the two k agree, and their rows go to the handles through the pointer table.  Different k: two searches (a search with the larger k
//     serving both is not used: that its prefix equals the shorter search in every rounding case has not been shown).
// Host waits of a call: one for the boxes, one per halving round that has to look at a count, one at the end (ctx->pp_waits counts them).
// prepare_plan.h splits the list into chunks and the rounds into groups whose cell tables fit.
#include "batch_dev.h"
#include "frontend.h"
#include "prims.h"
#include "prepare_plan.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int PP_SLOTS = 16;  // descriptor tables in flight between two host waits

// one pass over (some of) the clouds of a chunk: host -> device, one slot per pass
struct PpTab {
  int nb, pad_;
  int off[PP_MAX_CLOUDS + 1];       // points of the pass's clouds, concatenated in list order
  unsigned cb[PP_MAX_CLOUDS + 1];   // build: cell bases (prefix sums); scatter: the cloud's cell base in the build it is taken from
  unsigned tb[PP_MAX_CLOUDS + 1];   // scatter: table entries (ncell + 1 per cloud), prefix sums
  int src[PP_MAX_CLOUDS];           // first point of the cloud in the concatenated source array
  int soff[PP_MAX_CLOUDS];          // scatter: first sorted point of the cloud in the build it is taken from
  GridDesc g[PP_MAX_CLOUDS];
  const float4* ds[PP_MAX_CLOUDS];  // gather: the handles' down-sampled points
  float4* pts[PP_MAX_CLOUDS];       // scatter: the handles' grid buffers
  unsigned* start[PP_MAX_CLOUDS];
  float* nrm[PP_MAX_CLOUDS];        // k-NN pass: the handles' normals / covariances (null: not wanted)
  double* cov[PP_MAX_CLOUDS];
};

// boxes of the handles' down-sampled clouds (ctx.hip k_bbox per cloud: blockIdx.y + base is the cloud)
__global__ __launch_bounds__(256) void k_pp_bbox(const float4* const* __restrict__ ds, const int* __restrict__ m, int base, int* __restrict__ bb) {
  const int b = base + blockIdx.y;
  const float4* __restrict__ p = ds[b];
  const int n = m[b];
  float mn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, mx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float4 P = p[i];
    mn[0] = fminf(mn[0], P.x); mx[0] = fmaxf(mx[0], P.x);
    mn[1] = fminf(mn[1], P.y); mx[1] = fmaxf(mx[1], P.y);
    mn[2] = fminf(mn[2], P.z); mx[2] = fmaxf(mx[2], P.z);
  }
  gh_box_block(mn, mx, bb + (size_t)b * 6);
}

// the pass's clouds out of the handles into one array
__global__ __launch_bounds__(256) void k_pp_gather(const PpTab* __restrict__ T, int P, float4* __restrict__ cat) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const int j = fb_find(T->off, T->nb, i);
  cat[i] = T->ds[j][i - T->off[j]];
}

// grid.hip k_cell_keys per cloud, the cloud's cell base added; vals = index into the pass's concatenation
__global__ __launch_bounds__(256) void k_pp_cell_keys(const PpTab* __restrict__ T, const float4* __restrict__ cat, int P, unsigned* __restrict__ keys,
                                                      unsigned* __restrict__ vals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const int j = fb_find(T->off, T->nb, i);
  const GridDesc& g = T->g[j];
  const float4 Q = cat[T->src[j] + (i - T->off[j])];
  keys[i] = T->cb[j] + gh_cell_key(g, Q.x, Q.y, Q.z);
  vals[i] = (unsigned)i;
}

// icp.hip k_count_occupied with one counter per cloud: the first key of every run of equal sorted keys is an occupied cell of its cloud
__global__ __launch_bounds__(256) void k_pp_count_occupied(const PpTab* __restrict__ T, const unsigned* __restrict__ keys, int P, unsigned* __restrict__ cnt) {
  __shared__ unsigned s_cnt[PP_MAX_CLOUDS];
  if (threadIdx.x < PP_MAX_CLOUDS) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < P && (i == 0 || keys[i] != keys[i - 1])) atomicAdd(&s_cnt[fb_find(T->off, T->nb, i)], 1u);
  __syncthreads();
  if (threadIdx.x < T->nb && s_cnt[threadIdx.x] != 0u) atomicAdd(&cnt[threadIdx.x], s_cnt[threadIdx.x]);
}

// Out of a build into the handles: threads [0, P) write the clouds' sorted points (grid.hip k_gather_sorted, w = the point's index in ITS
// cloud), threads [P, P + E) their slices of the cell table (ncell + 1 entries each, counted from the cloud's first sorted point).
__global__ __launch_bounds__(256) void k_pp_scatter(const PpTab* __restrict__ T, const float4* __restrict__ cat, const unsigned* __restrict__ vals,
                                                    const unsigned* __restrict__ gstart, unsigned P, unsigned E) {
  const unsigned long long t = blockIdx.x * 256ull + threadIdx.x;
  if (t < P) {
    const int i = (int)t;
    const int w = fb_find(T->off, T->nb, i), j = i - T->off[w];
    const int local = (int)vals[T->soff[w] + j] - T->soff[w];
    const float4 Q = cat[T->src[w] + local];
    T->pts[w][j] = make_float4(Q.x, Q.y, Q.z, __uint_as_float((unsigned)local));
  } else if (t - P < E) {
    const unsigned e = (unsigned)(t - P);
    const int w = fb_find(T->tb, T->nb, e);
    const unsigned c = e - T->tb[w];
    T->start[w][c] = gstart[T->cb[w] + c] - (unsigned)T->soff[w];
  }
}

// rows of the k-NN pass into the handles that asked for them
__global__ __launch_bounds__(256) void k_pp_scatter_rows(const PpTab* __restrict__ T, const float* __restrict__ nrm, const double* __restrict__ cov, int P) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const int w = fb_find(T->off, T->nb, i);
  const size_t j = (size_t)(i - T->off[w]);
  float* dn = T->nrm[w];
  double* dc = T->cov[w];
  if (nrm && dn) { dn[j * 3] = nrm[(size_t)i * 3]; dn[j * 3 + 1] = nrm[(size_t)i * 3 + 1]; dn[j * 3 + 2] = nrm[(size_t)i * 3 + 2]; }
  if (cov && dc)
    for (int e = 0; e < 6; e++) dc[j * 6 + e] = cov[(size_t)i * 6 + e];
}

// one cloud with device work in this call
struct PpCloud {
  ghicp_cloud* c;
  int m;
  bool grids, nrm, cov, ov;
  float mm[6];
  GridDesc fine0, knn, ovg;  // fine grid at its start cell, k-NN grid, overlap grid
  float cell0;
};

const GridSlots kSlotsA = {B_GRID_KEYS, B_GRID_KEYS2, B_GRID_VALS, B_GRID_VALS2, B_GRID_START, B_GRID_PTS};
const GridSlots kSlotsB = {B_GRID2_KEYS, B_GRID2_KEYS2, B_GRID2_VALS, B_GRID2_VALS2, B_GRID2_START, B_GRID2_PTS};

struct Built {  // a build in the context's buffers
  PpTab H;   // host copy of its table (the pinned slot it was uploaded from is free again after the next host wait)
  PpTab* D;
  int P;
  unsigned cells;
  const unsigned *keys, *vals, *start;
};

struct PpRun {
  ghicp_ctx* ctx;
  hipStream_t s;
  const ghicp_prepare_spec* spec;
  PpTab *Hbase = nullptr, *Dbase = nullptr;
  unsigned *Hcnt = nullptr, *Dcnt = nullptr;
  int used = 0;

  int begin() {
    const size_t bytes = sizeof(PpTab) * PP_SLOTS + sizeof(unsigned) * PP_MAX_CLOUDS;
    if (!ctx->pp_pinned && hipHostMalloc(&ctx->pp_pinned, bytes, hipHostMallocDefault) != hipSuccess)
      return ctx->fail(GHICP_ERR_HIP, "ghicp_clouds_prepare: pinned allocation failed");
    char* d;
    GH_TRY(ctx->reserve(B_PP_DESC, bytes, &d));
    Hbase = reinterpret_cast<PpTab*>(ctx->pp_pinned);
    Dbase = reinterpret_cast<PpTab*>(d);
    Hcnt = reinterpret_cast<unsigned*>(Hbase + PP_SLOTS);
    Dcnt = reinterpret_cast<unsigned*>(Dbase + PP_SLOTS);
    return GHICP_OK;
  }
  int wait() {  // a host synchronisation; every slot is free again afterwards
    GH_HIP(hipStreamSynchronize(s));
    ctx->pp_waits++;
    used = 0;
    return GHICP_OK;
  }
  int tab(PpTab** h, PpTab** d) {
    if (used == PP_SLOTS) GH_TRY(wait());
    *h = Hbase + used; *d = Dbase + used;
    used++;
    memset(*h, 0, sizeof(PpTab));
    return GHICP_OK;
  }
  int upload(PpTab* h, PpTab* d) {
    GH_HIP(hipMemcpyAsync(d, h, sizeof(PpTab), hipMemcpyHostToDevice, s));
    return GHICP_OK;
  }

  // global cell keys -> stable sort -> cell table for the clouds `who` (indices into W) with the descriptors gd; their points are read from
  // `cat` at srcoff[]
  int build(const PpCloud* W, const std::vector<int>& who, const std::vector<GridDesc>& gd, const float4* cat, const std::vector<int>& srcoff,
            const GridSlots& sl, Built* out) {
    PpTab *H, *D;
    GH_TRY(tab(&H, &D));
    const int nb = (int)who.size();
    H->nb = nb;
    unsigned long long cells = 0;
    for (int j = 0; j < nb; j++) {
      H->off[j + 1] = H->off[j] + W[who[j]].m;
      H->cb[j] = (unsigned)cells;
      cells += gd[j].ncell;
      H->src[j] = srcoff[j];
      H->g[j] = gd[j];
    }
    H->cb[nb] = (unsigned)cells;
    const int P = H->off[nb];
    GridBufs B;
    GH_TRY(gh_grid_reserve(ctx, sl, (size_t)P, (size_t)cells, false, &B));  // the points go to the handles (scatter) or to the k-NN pass's own buffer
    GH_TRY(upload(H, D));
    hipLaunchKernelGGL(k_pp_cell_keys, dim3(cdiv(P, 256)), dim3(256), 0, s, (const PpTab*)D, cat, P, B.keys, B.vals);
    GH_TRY(gh_radix_sort_u32(ctx, B.keys, B.keys2, B.vals, B.vals2, P, 0, bits_for(cells)));  // stable: a cell keeps its points in down-sampled order (prims.hip)
    gh_cell_start_launch(s, B.keys2, (unsigned)P, (unsigned)cells, B.start);
    GH_HIP(hipGetLastError());
    out->H = *H; out->D = D; out->P = P; out->cells = (unsigned)cells; out->keys = B.keys2; out->vals = B.vals2; out->start = B.start;
    return GHICP_OK;
  }

  // the grids of the build's clouds picked[] (positions in the build) into the handles' buffers pts_of / start_of
  int scatter(const Built& B, const std::vector<int>& picked, const float4* cat, const std::vector<float4*>& pts, const std::vector<unsigned*>& start) {
    if (picked.empty()) return GHICP_OK;
    PpTab *H, *D;
    GH_TRY(tab(&H, &D));
    const int nw = (int)picked.size();
    H->nb = nw;
    for (int w = 0; w < nw; w++) {
      const int j = picked[w];
      const int mj = B.H.off[j + 1] - B.H.off[j];
      H->off[w + 1] = H->off[w] + mj;
      H->tb[w + 1] = H->tb[w] + B.H.g[j].ncell + 1u;
      H->cb[w] = B.H.cb[j];
      H->soff[w] = B.H.off[j];
      H->src[w] = B.H.src[j];
      H->pts[w] = pts[w];
      H->start[w] = start[w];
    }
    GH_TRY(upload(H, D));
    const unsigned P = (unsigned)H->off[nw], E = H->tb[nw];
    hipLaunchKernelGGL(k_pp_scatter, dim3((unsigned)cdiv((long long)P + E, 256)), dim3(256), 0, s, (const PpTab*)D, cat, B.vals, B.start, P, E);
    GH_HIP(hipGetLastError());
    return GHICP_OK;
  }

  int boxes(std::vector<PpCloud>& W);
  int chunk(PpCloud* W, int nb);
  int fine_rounds(PpCloud* W, const std::vector<int>& F, const float4* cat, const std::vector<int>& moff);
  int grid_kind(PpCloud* W, const std::vector<int>& who, int kind, const float4* cat, const std::vector<int>& moff);
  int knn_pass(PpCloud* W, int nb, int k, bool want_n, bool want_c, const float4* cat);
};

// ------------------------------------------------------------------ boxes of every cloud with device work            (one host wait)
int PpRun::boxes(std::vector<PpCloud>& W) {
  const size_t n = W.size();
  const size_t bytes = n * (sizeof(void*) + sizeof(int)) + 8;
  std::vector<char> host(bytes);
  const float4** hp = reinterpret_cast<const float4**>(host.data());
  int* hm = reinterpret_cast<int*>(host.data() + n * sizeof(void*));
  int maxm = 1;
  for (size_t i = 0; i < n; i++) { hp[i] = W[i].c->ds.as<float4>(); hm[i] = W[i].m; maxm = std::max(maxm, W[i].m); }
  char* d;
  GH_TRY(ctx->reserve(B_PP_BOX, bytes + n * 6 * sizeof(int) + 64, &d));
  int* bb = reinterpret_cast<int*>(d + ((bytes + 15) & ~(size_t)15));
  GH_TRY(ctx->upload_table(host.data(), bytes, d));
  hipLaunchKernelGGL(k_box_init, dim3(cdiv((long long)n * 6, 256)), dim3(256), 0, s, bb, (int)(n * 6));
  const int bx = std::min(cdiv(maxm, 256), 64);
  for (size_t base = 0; base < n; base += 32768) {
    const unsigned ny = (unsigned)std::min<size_t>(32768, n - base);
    hipLaunchKernelGGL(k_pp_bbox, dim3(bx, ny), dim3(256), 0, s, reinterpret_cast<const float4* const*>(d), reinterpret_cast<const int*>(d + n * sizeof(void*)),
                       (int)base, bb);
  }
  GH_HIP(hipGetLastError());
  std::vector<int> enc(n * 6);
  GH_HIP(hipMemcpyAsync(enc.data(), bb, n * 6 * sizeof(int), hipMemcpyDeviceToHost, s));
  GH_TRY(wait());
  for (size_t i = 0; i < n; i++) {
    PpCloud& C = W[i];
    gh_box_decode(enc.data() + i * 6, C.mm);
    const float* mm = C.mm;
    memset(&C.fine0, 0, sizeof(GridDesc)); memset(&C.knn, 0, sizeof(GridDesc)); memset(&C.ovg, 0, sizeof(GridDesc));
    if (C.grids) {  // the start cell of icp.hip build_index
      const double vol = fmax(1e-9, (double)(mm[3] - mm[0] + 1e-3) * (mm[4] - mm[1] + 1e-3) * (mm[5] - mm[2] + 1e-3));
      C.cell0 = fmaxf((float)cbrt(vol / (double)C.m * 8.0), 0.02f);
      C.fine0 = gh_grid_desc(mm, C.m, C.cell0);
    }
    if (C.nrm || C.cov) C.knn = gh_grid_desc(mm, C.m, gh_fpfh_cell(mm, C.m));  // fpfh.hip knn_lists
    if (C.ov) C.ovg = gh_grid_desc(mm, C.m, spec->thre_dis);
  }
  return GHICP_OK;
}

// ------------------------------------------------------------------ the fine grids: halving rounds      (a host wait per round with a count)
int PpRun::fine_rounds(PpCloud* W, const std::vector<int>& F, const float4* cat, const std::vector<int>& moff) {
  struct St { int w; float cell; int attempt; GridDesc g; };
  std::vector<St> active;
  for (int w : F) active.push_back({w, W[w].cell0, 0, W[w].fine0});
  while (!active.empty()) {
    // the clouds of this round: the leading ones whose grids fit one cell table together (all of them, unless the clouds are very large)
    std::vector<PpSize> sz(active.size());
    for (size_t a = 0; a < active.size(); a++) sz[a] = {W[active[a].w].m, {active[a].g.ncell, 0, 0}};
    const int take = pp_prefix(sz.data(), (int)sz.size());
    std::vector<int> who(take), srcoff(take);
    std::vector<GridDesc> gd(take);
    for (int a = 0; a < take; a++) { who[a] = active[a].w; gd[a] = active[a].g; srcoff[a] = moff[active[a].w]; }
    Built B;
    GH_TRY(build(W, who, gd, cat, srcoff, kSlotsA, &B));
    // the stop rules of build_index, per cloud: the first three need no count
    std::vector<char> stop(take, 0);
    bool need_count = false;
    for (int a = 0; a < take; a++) {
      const St& S = active[a];
      const double nc_next = (double)S.g.dim[0] * S.g.dim[1] * S.g.dim[2] * 8.0;
      if (S.attempt >= 5 || nc_next > (double)(1u << 26) || 1.0f / S.g.inv > S.cell * 1.01f) stop[a] = 1;
      else need_count = true;
    }
    if (need_count) {
      GH_HIP(hipMemsetAsync(Dcnt, 0, sizeof(unsigned) * PP_MAX_CLOUDS, s));
      hipLaunchKernelGGL(k_pp_count_occupied, dim3(cdiv(B.P, 256)), dim3(256), 0, s, (const PpTab*)B.D, B.keys, B.P, Dcnt);
      GH_HIP(hipMemcpyAsync(Hcnt, Dcnt, sizeof(unsigned) * PP_MAX_CLOUDS, hipMemcpyDeviceToHost, s));
      GH_TRY(wait());
      for (int a = 0; a < take; a++)
        if (!stop[a]) {
          const unsigned occ = Hcnt[a];
          if (occ == 0 || (double)W[active[a].w].m / occ <= 8.0) stop[a] = 1;
        }
    }
    // the clouds that stop keep the grid of this round
    std::vector<int> picked;
    std::vector<float4*> pts;
    std::vector<unsigned*> start;
    for (int a = 0; a < take; a++)
      if (stop[a]) {
        ghicp_cloud* c = W[active[a].w].c;
        GH_HIP(c->rf_fstart.reserve(((size_t)active[a].g.ncell + 1) * sizeof(unsigned)));
        picked.push_back(a); pts.push_back(c->rf_fpts.as<float4>()); start.push_back(c->rf_fstart.as<unsigned>());
        c->rf_fine = active[a].g;
      }
    GH_TRY(scatter(B, picked, cat, pts, start));
    std::vector<St> next;
    for (size_t a = 0; a < active.size(); a++) {
      if ((int)a < take) {
        if (stop[a]) continue;
        St S = active[a];
        S.cell *= 0.5f;
        S.attempt++;
        S.g = gh_grid_desc(W[S.w].mm, W[S.w].m, S.cell);
        next.push_back(S);
      } else next.push_back(active[a]);
    }
    active.swap(next);
  }
  return GHICP_OK;
}

// ------------------------------------------------------------------ coarse grids (kind 0) / overlap grids (kind 1): no host wait
int PpRun::grid_kind(PpCloud* W, const std::vector<int>& who_all, int kind, const float4* cat, const std::vector<int>& moff) {
  size_t done = 0;
  while (done < who_all.size()) {
    const size_t left = who_all.size() - done;
    std::vector<PpSize> sz(left);
    std::vector<GridDesc> gd_all(left);
    for (size_t a = 0; a < left; a++) {
      const PpCloud& C = W[who_all[done + a]];
      gd_all[a] = kind == 0 ? gh_grid_desc(C.mm, C.m, (1.0f / C.c->rf_fine.inv) * 8.0f) : C.ovg;  // coarse: 8 x the fine cell actually used
      sz[a] = {C.m, {gd_all[a].ncell, 0, 0}};
    }
    const int take = pp_prefix(sz.data(), (int)left);
    std::vector<int> who(take), srcoff(take), picked(take);
    std::vector<GridDesc> gd(take);
    std::vector<float4*> pts(take);
    std::vector<unsigned*> start(take);
    for (int a = 0; a < take; a++) {
      who[a] = who_all[done + a]; gd[a] = gd_all[a]; srcoff[a] = moff[who[a]]; picked[a] = a;
      ghicp_cloud* c = W[who[a]].c;
      DevBuf& bs = kind == 0 ? c->rf_cstart : c->ov_start;
      GH_HIP(bs.reserve(((size_t)gd[a].ncell + 1) * sizeof(unsigned)));
      pts[a] = (kind == 0 ? c->rf_cpts : c->ov_pts).as<float4>();
      start[a] = bs.as<unsigned>();
      (kind == 0 ? c->rf_coarse : c->ov_grid) = gd[a];
    }
    Built B;
    GH_TRY(build(W, who, gd, cat, srcoff, kSlotsA, &B));
    GH_TRY(scatter(B, picked, cat, pts, start));
    done += (size_t)take;
  }
  return GHICP_OK;
}

// ------------------------------------------------------------------ one k-NN search; normals and / or covariances over its lists
int PpRun::knn_pass(PpCloud* W, int nb, int k, bool want_n, bool want_c, const float4* cat) {
  std::vector<int> who;
  for (int b = 0; b < nb; b++)
    if ((want_n && W[b].nrm) || (want_c && W[b].cov)) who.push_back(b);
  if (who.empty()) return GHICP_OK;
  const int ns = (int)who.size();
  hipEvent_t kt = ctx->kt_begin(KT_PP_KNN);
  std::vector<GridDesc> gd(ns);
  std::vector<int> srcoff(ns);
  int P = 0;
  for (int j = 0; j < ns; j++) { gd[j] = W[who[j]].knn; srcoff[j] = P; P += W[who[j]].m; }
  const float4* catk = cat;
  if (ns != nb) {  // the pass's clouds alone, concatenated (all clouds of the chunk: the chunk's array is that already)
    PpTab *H, *D;
    GH_TRY(tab(&H, &D));
    H->nb = ns;
    for (int j = 0; j < ns; j++) { H->off[j + 1] = H->off[j] + W[who[j]].m; H->ds[j] = W[who[j]].c->ds.as<float4>(); }
    float4* ck;
    GH_TRY(ctx->reserve(B_PP_CATK, (size_t)P + 1, &ck));
    GH_TRY(upload(H, D));
    hipLaunchKernelGGL(k_pp_gather, dim3(cdiv(P, 256)), dim3(256), 0, s, (const PpTab*)D, P, ck);
    catk = ck;
  }
  Built B;
  GH_TRY(build(W, who, gd, catk, srcoff, kSlotsB, &B));
  float4* pts;
  GH_TRY(ctx->reserve(B_GRID2_PTS, (size_t)P + 1, &pts));
  hipLaunchKernelGGL(k_gather_sorted_f4, dim3(cdiv(P, 256)), dim3(256), 0, s, catk, B.vals, P, pts);  // w = index into the pass's concatenation
  float* nrm = nullptr;
  double* cov = nullptr;
  if (want_n) GH_TRY(ctx->reserve(B_PP_NRM, (size_t)P * 3 + 3, &nrm));
  if (want_c) GH_TRY(ctx->reserve(B_PP_COV, (size_t)P * 6 + 6, &cov));
  GH_TRY(gh_knn_prepare_batch_dev(ctx, catk, P, pts, B.start, B.D->g, B.D->cb, B.D->off, ns, k, nrm, spec->gicp_epsilon, cov));
  PpTab *H, *D;
  GH_TRY(tab(&H, &D));
  H->nb = ns;
  for (int j = 0; j < ns; j++) {
    const PpCloud& C = W[who[j]];
    H->off[j + 1] = H->off[j] + C.m;
    H->nrm[j] = (want_n && C.nrm) ? C.c->rf_nrm.as<float>() : nullptr;
    H->cov[j] = (want_c && C.cov) ? C.c->gc_cov.as<double>() : nullptr;
  }
  GH_TRY(upload(H, D));
  hipLaunchKernelGGL(k_pp_scatter_rows, dim3(cdiv(P, 256)), dim3(256), 0, s, (const PpTab*)D, (const float*)nrm, (const double*)cov, P);
  GH_HIP(hipGetLastError());
  ctx->kt_end(KT_PP_KNN, kt);
  return GHICP_OK;
}

// ------------------------------------------------------------------ one chunk: one launch sequence
int PpRun::chunk(PpCloud* W, int nb) {
  std::vector<int> moff(nb + 1, 0), F, O;
  bool any_n = false, any_c = false;
  for (int b = 0; b < nb; b++) {
    moff[b + 1] = moff[b] + W[b].m;
    if (W[b].grids) F.push_back(b);
    if (W[b].ov) O.push_back(b);
    any_n = any_n || W[b].nrm;
    any_c = any_c || W[b].cov;
  }
  const int M = moff[nb];
  // the handles' buffers whose sizes are known now (the cell tables are reserved when their grid is final)
  for (int b = 0; b < nb; b++) {
    ghicp_cloud* c = W[b].c;
    if (W[b].grids) { GH_HIP(c->rf_fpts.reserve((size_t)W[b].m * sizeof(float4))); GH_HIP(c->rf_cpts.reserve((size_t)W[b].m * sizeof(float4))); }
    if (W[b].ov) GH_HIP(c->ov_pts.reserve((size_t)W[b].m * sizeof(float4)));
  }
  float4* cat;
  GH_TRY(ctx->reserve(B_PP_CAT, (size_t)M + 1, &cat));
  {
    PpTab *H, *D;
    GH_TRY(tab(&H, &D));
    H->nb = nb;
    for (int b = 0; b < nb; b++) { H->off[b + 1] = moff[b + 1]; H->ds[b] = W[b].c->ds.as<float4>(); }
    GH_TRY(upload(H, D));
    hipLaunchKernelGGL(k_pp_gather, dim3(cdiv(M, 256)), dim3(256), 0, s, (const PpTab*)D, M, cat);
    GH_HIP(hipGetLastError());
  }
  hipEvent_t kg = ctx->kt_begin(KT_PP_GRIDS);
  if (!F.empty()) {
    GH_TRY(fine_rounds(W, F, cat, moff));
    GH_TRY(grid_kind(W, F, 0, cat, moff));
  }
  if (!O.empty()) GH_TRY(grid_kind(W, O, 1, cat, moff));
  ctx->kt_end(KT_PP_GRIDS, kg);
  if (any_n && any_c && spec->normals_k == spec->gicp_k) GH_TRY(knn_pass(W, nb, spec->gicp_k, true, true, cat));
  else {
    if (any_n) GH_TRY(knn_pass(W, nb, spec->normals_k, true, false, cat));
    if (any_c) GH_TRY(knn_pass(W, nb, spec->gicp_k, false, true, cat));
  }
  return GHICP_OK;
}

void grid_info(const GridDesc& g, ghicp_grid_info* o) {
  memset(o, 0, sizeof(*o));
  for (int d = 0; d < 3; d++) { o->mn[d] = g.mn[d]; o->dim[d] = g.dim[d]; }
  o->inv = g.inv; o->n = g.n; o->ncell = g.ncell;
}

}  // namespace

extern "C" int ghicp_prepare_spec_default(ghicp_prepare_spec* s) {
  if (!s) return GHICP_ERR_ARG;
  memset(s, 0, sizeof(*s));
  s->gicp_epsilon = 1e-3;
  s->thre_dis = 0.5f;
  return GHICP_OK;
}

extern "C" int ghicp_ctx_prepare_host_waits(const ghicp_ctx* ctx, int64_t* waits) {
  if (!ctx || !waits) return GHICP_ERR_ARG;
  *waits = ctx->pp_waits;
  return GHICP_OK;
}

extern "C" int ghicp_clouds_prepare(ghicp_ctx* ctx, int32_t n_clouds, ghicp_cloud* const* clouds, const ghicp_prepare_spec* spec) {
  GH_ENTER(ctx);
  GH_ARG(spec != nullptr && n_clouds >= 0 && (n_clouds == 0 || clouds != nullptr));
  GH_ARG(spec->normals_k >= 0 && spec->normals_k <= 20 && spec->gicp_k >= 0 && spec->gicp_k <= 20);
  const int nk = spec->normals_k, gk = spec->gicp_k;
  const bool do_ref = spec->refine != 0 || nk > 0, do_g = gk > 0, do_ov = spec->overlap != 0;
  if (do_ov) GH_ARG(spec->thre_dis > 0.f);
  if (do_g) GH_ARG(spec->gicp_epsilon > 0.0);
  // every handle is checked before anything is touched or launched
  for (int i = 0; i < n_clouds; i++) {
    GH_ARG(clouds[i] != nullptr && clouds[i]->ctx == ctx);
    if (!clouds[i]->ds.p) return ctx->fail(GHICP_ERR_ARG, "ghicp_clouds_prepare: cloud %d was rebuilt from stored features and holds no points", i);
  }
  {
    std::vector<const ghicp_cloud*> sorted(clouds, clouds + n_clouds);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return ctx->fail(GHICP_ERR_ARG, "ghicp_clouds_prepare: a handle is listed twice");
  }
  ctx->pp_waits = 0;
  if (n_clouds == 0 || !(do_ref || do_g || do_ov)) return GHICP_OK;
  if (ctx->host_ptrs) {  // cloud by cloud, as the batched front end does in this mode
    for (int i = 0; i < n_clouds; i++) {
      if (do_ref) GH_TRY(ghicp_cloud_prepare_refine(clouds[i], nk));
      if (do_g) GH_TRY(ghicp_cloud_prepare_gicp(clouds[i], gk, spec->gicp_epsilon));
      if (do_ov) GH_TRY(ghicp_cloud_prepare_overlap(clouds[i], spec->thre_dis));
    }
    return GHICP_OK;
  }
  // what each handle needs under the keep / replace rules of the three per-cloud calls, and the state it ends in
  std::vector<PpCloud> W;
  std::vector<int> final_rf_k((size_t)n_clouds);
  for (int i = 0; i < n_clouds; i++) {
    ghicp_cloud* c = clouds[i];
    PpCloud C;
    memset(&C, 0, sizeof(C));
    C.c = c; C.m = (int)c->m;
    C.grids = (do_ref || do_g) && !c->rf_ready;
    C.nrm = do_ref && nk > 0 && (nk != c->rf_k || !c->rf_ready);
    C.cov = do_g && !(c->gc_ready && c->gc_k == gk && c->gc_eps == spec->gicp_epsilon);
    C.ov = do_ov && !(c->ov_ready && c->ov_thre == spec->thre_dis);
    final_rf_k[i] = do_ref ? nk : ((do_g && !c->rf_ready) ? 0 : c->rf_k);
    // invalid until everything below is in place
    if (do_ref || (do_g && !c->rf_ready)) c->rf_invalidate();
    if (do_g) c->gc_invalidate();
    if (C.ov) c->ov_invalidate();
    if (C.grids) { memset(&c->rf_fine, 0, sizeof(GridDesc)); memset(&c->rf_coarse, 0, sizeof(GridDesc)); }
    if (C.ov) memset(&c->ov_grid, 0, sizeof(GridDesc));
    if (C.nrm) GH_HIP(c->rf_nrm.reserve(((size_t)c->m * 3 + 3) * sizeof(float)));
    if (C.cov && c->m > 0) GH_HIP(c->gc_cov.reserve(((size_t)c->m * 6 + 6) * sizeof(double)));
    if (c->m > 0 && (C.grids || C.nrm || C.cov || C.ov)) W.push_back(C);  // an empty cloud launches nothing: zeroed descriptors, flags set
  }
  PpRun R;
  R.ctx = ctx; R.s = ctx->stream; R.spec = spec;
  if (!W.empty()) {
    GH_TRY(R.begin());
    GH_TRY(R.boxes(W));
    std::vector<PpSize> sz(W.size());
    for (size_t i = 0; i < W.size(); i++) sz[i] = {W[i].m, {W[i].fine0.ncell, W[i].knn.ncell, W[i].ovg.ncell}};
    for (const PpChunk& ch : pp_plan(sz.data(), (int)sz.size())) GH_TRY(R.chunk(W.data() + ch.first, ch.count));
    GH_TRY(R.wait());  // afterwards the handles may serve any context of the device
  }
  for (int i = 0; i < n_clouds; i++) {
    ghicp_cloud* c = clouds[i];
    if (do_ref || do_g) { c->rf_k = final_rf_k[i]; c->rf_ready = true; }
    if (do_g) { c->gc_k = gk; c->gc_eps = spec->gicp_epsilon; c->gc_ready = true; }
    if (do_ov) { c->ov_thre = spec->thre_dis; c->ov_ready = true; }
  }
  return GHICP_OK;
}

extern "C" int ghicp_cloud_get_prepared(const ghicp_cloud* c, ghicp_cloud_prepared* out) {
  if (!c || !out) return GHICP_ERR_ARG;
  memset(out, 0, sizeof(*out));
  out->refine_ready = c->rf_ready ? 1 : 0; out->normals_k = c->rf_k;
  out->gicp_ready = c->gc_ready ? 1 : 0; out->gicp_k = c->gc_k; out->gicp_epsilon = c->gc_eps;
  out->overlap_ready = c->ov_ready ? 1 : 0; out->thre_dis = c->ov_thre;
  if (c->rf_ready) { grid_info(c->rf_fine, &out->fine); grid_info(c->rf_coarse, &out->coarse); }
  if (c->ov_ready) grid_info(c->ov_grid, &out->overlap);
  return GHICP_OK;
}

extern "C" int ghicp_cloud_download_prepared(const ghicp_cloud* c, int32_t which, void* out) {
  if (!c || !c->ctx) return GHICP_ERR_ARG;
  ghicp_ctx* ctx = c->ctx;
  GH_ENTER(ctx);
  GH_ARG(which >= GHICP_PREP_FINE_PTS && which <= GHICP_PREP_COVARIANCES);
  const void* src = nullptr;
  size_t bytes = 0;
  bool held = false;
  const size_t m = (size_t)c->m;
  switch (which) {
    case GHICP_PREP_FINE_PTS: held = c->rf_ready; src = c->rf_fpts.p; bytes = m * sizeof(float4); break;
    case GHICP_PREP_FINE_START: held = c->rf_ready; src = c->rf_fstart.p; bytes = ((size_t)c->rf_fine.ncell + 1) * sizeof(unsigned); break;
    case GHICP_PREP_COARSE_PTS: held = c->rf_ready; src = c->rf_cpts.p; bytes = m * sizeof(float4); break;
    case GHICP_PREP_COARSE_START: held = c->rf_ready; src = c->rf_cstart.p; bytes = ((size_t)c->rf_coarse.ncell + 1) * sizeof(unsigned); break;
    case GHICP_PREP_OVERLAP_PTS: held = c->ov_ready; src = c->ov_pts.p; bytes = m * sizeof(float4); break;
    case GHICP_PREP_OVERLAP_START: held = c->ov_ready; src = c->ov_start.p; bytes = ((size_t)c->ov_grid.ncell + 1) * sizeof(unsigned); break;
    case GHICP_PREP_NORMALS: held = c->rf_ready && c->rf_k > 0; src = c->rf_nrm.p; bytes = m * 3 * sizeof(float); break;
    default: held = c->gc_ready; src = c->gc_cov.p; bytes = m * 6 * sizeof(double); break;
  }
  if (!held) return ctx->fail(GHICP_ERR_ARG, "ghicp_cloud_download_prepared: the handle does not hold part %d", (int)which);
  if (m == 0) return GHICP_OK;  // an empty cloud holds no buffers
  GH_ARG(out != nullptr && src != nullptr);
  GH_HIP(hipMemcpyAsync(out, src, bytes, ctx->host_ptrs ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
  GH_HIP(hipStreamSynchronize(ctx->stream));
  return GHICP_OK;
}
