// Stand-alone driver of the chunk planner of ghicp_clouds_prepare (pp_plan / pp_prefix, gh-icp_amd/csrc/prepare_plan.h), built by
// tests/test_prepare_clouds_cpu.py (also with -fsanitize=address,undefined).  Reads cases from stdin -- "n max_clouds max_points max_cells"
// followed by n lines "m cells0 cells1 cells2" (max_clouds 0: the library's limits) -- and prints for each case its chunks "first count", one
// per line, then "end".  The test compares them with its own restatement of the rule and checks cover, order and limits.
#include <cstdio>
#include <cstdlib>

#include "prepare_plan.h"

int main() {
  int n, max_clouds;
  long long max_points;
  unsigned long long max_cells;
  while (scanf("%d %d %lld %llu", &n, &max_clouds, &max_points, &max_cells) == 4) {
    if (n < 0) return 2;
    // a heap copy of exactly n entries: a read past the list aborts under AddressSanitizer
    PpSize* sz = (PpSize*)malloc(sizeof(PpSize) * (size_t)(n > 0 ? n : 1));
    for (int i = 0; i < n; i++)
      if (scanf("%lld %llu %llu %llu", &sz[i].m, &sz[i].cells[0], &sz[i].cells[1], &sz[i].cells[2]) != 4) return 2;
    PpLimits L;
    if (max_clouds > 0) { L.max_clouds = max_clouds; L.max_points = max_points; L.max_cells = max_cells; }
    for (const PpChunk& c : pp_plan(sz, n, L)) printf("%d %d\n", c.first, c.count);
    printf("end\n");
    free(sz);
  }
  return 0;
}
