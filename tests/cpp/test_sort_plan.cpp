// Stand-alone driver of the segmented radix sort's host plan (gh_rs_plan / gh_rs_segs_make, gh-icp_amd/csrc/sort_plan.h), built by
// tests/test_sort_segments_cpu.py (also with -fsanitize=address,undefined).  Reads lines from stdin:
//   "p bits max_width"        -> prints "places w0 w1 ..."
//   "s nseg off0 .. off_nseg" -> prints "longest", then one line "off toff coff" per entry 0 .. nseg
// The test compares both with its own restatement of the rules.
#include <cstdio>
#include <cstdlib>

#include "sort_plan.h"

int main() {
  char what;
  while (scanf(" %c", &what) == 1) {
    if (what == 'p') {
      int bits, width;
      if (scanf("%d %d", &bits, &width) != 2) return 2;
      const GhRsPlan P = gh_rs_plan(bits, width);
      printf("%d", P.places);
      for (int p = 0; p < P.places; p++) printf(" %d", P.width[p]);
      printf("\n");
    } else if (what == 's') {
      int nseg;
      if (scanf("%d", &nseg) != 1 || nseg < 1 || nseg > GH_RS_MAX_SEGS) return 2;
      // a heap copy of exactly nseg + 1 entries: a read past the list aborts under AddressSanitizer
      long long* off = (long long*)malloc(sizeof(long long) * (size_t)(nseg + 1));
      for (int i = 0; i <= nseg; i++)
        if (scanf("%lld", &off[i]) != 1) return 2;
      GhRsSegs* S = (GhRsSegs*)malloc(sizeof(GhRsSegs));
      printf("%lld\n", gh_rs_segs_make(S, nseg, off));
      for (int i = 0; i <= nseg; i++) printf("%d %d %d\n", S->off[i], S->toff[i], S->coff[i]);
      free(S);
      free(off);
    } else return 2;
  }
  return 0;
}
