// Internal: descriptor of one sparse Kuhn-Munkres problem (shared by loop.hip, km_dense_door.hip, km4.hip).  Not part of the ABI.
#pragma once
struct Km2Problem {
  int n, pad_;
  double bg, eps;
  const unsigned* row_ptr;  // n+1
  const int* cols;          // ascending within a row
  const double* vals;       // explicit weights, each > bg
  const double* lx_init;    // row maxima over the full row (km.cpp:56-62)
  int* match_out;           // n: match[y] = x
  int* status;              // 0 = ok
  const int* done;          // optional early-exit flag (device)
  long long* steps;         // optional: counters (profiling)
};
struct ghicp_ctx;
int gh_km4_launch(ghicp_ctx* ctx, const Km2Problem* d_probs, int nprob, int n_max);
bool gh_km4_fits(int n);
size_t gh_km4_lds_bytes(int n);
size_t gh_km4_lds_bytes_compact(int n);              // the compact layout (km4_dev.h): sty and tlo in a per-slot global region
size_t gh_km4_slot_bytes(int n, bool compact_on);    // what a solve slot asks for: compact only where that makes the graph four per CU
// Test-only exports of the library (km4.hip; host code, no device work; NOT part of the C ABI in include/ghicp_c.h and absent from api.EXPORTS):
// the classes gh_km4_plan forms for `count` graphs of n[] rows, and gh_km4_lds_bytes / gh_km4_lds_bytes_compact.
extern "C" int ghicp_km4_plan_probe(const int32_t* n, int32_t count, int32_t compact_on, int32_t* per_cu_of_problem, int64_t* lds_of_class, int32_t* nclass);
extern "C" int64_t ghicp_km4_lds_bytes(int32_t n, int32_t compact);

// A batch of problems of different sizes: problems are grouped into classes of equal LDS occupancy (problems per CU) so that one
// large problem does not lower the occupancy of all the others, and within a class the largest problems start first.
struct Km4Plan {
  int nclass = 0;
  int begin[8] = {0}, count[8] = {0};
  size_t lds[8] = {0};
  int per_cu[8] = {0};      // problems per CU of the class by LDS (capped at four)
  int nmax[8] = {0};        // the class's largest graph
  double weight[8] = {0};   // the class's share of the batch's work: sum of the cost hints, or of n^2 without hints
  int* d_order = nullptr;  // device: problem indices, class after class
};
// cost: optional per-problem cost hints (host, nprob floats): within a class the costliest problems are queued first
int gh_km4_plan(ghicp_ctx* ctx, const int* h_n, int nprob, Km4Plan* plan, const float* cost = nullptr);
int gh_km4_launch_plan(ghicp_ctx* ctx, const Km2Problem* d_probs, const Km4Plan& plan);
