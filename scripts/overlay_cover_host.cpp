// The overlay's coverage rules (pmce_amd/csrc/overlay_cover.hpp) on the host: reads cases from a text file, prints one verdict per
// line.  tests/test_overlay_host.py compares the verdicts with Python integers, so the 128-bit arithmetic of the segment rule is checked
// without a GPU.  Built with the host compiler:  c++ -std=c++17 -O1 -I pmce_amd/csrc scripts/overlay_cover_host.cpp -o overlay_cover_host
//
// A case is one line:
//   Q <bits>                        quantise(v), v the fp64 whose 64 bits are <bits> (hexadecimal)      -> "<guard> <q>"
//                                   guard = 1: beyond the guard band (or not a number); q is then 0
//   S ax ay bx by cx cy thickness   segment_covers, coordinates in 1/16 px                               -> "0" or "1"
//   D kx ky cx cy radius            disc_covers                                                          -> "0" or "1"
//   C lo hi n                       centre_span                                                          -> "<p0> <p1>"
#include <stdio.h>
#include <string.h>

#include "overlay_cover.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s cases.txt\n", argv[0]);
    return 2;
  }
  FILE* fh = fopen(argv[1], "r");
  if (!fh) {
    fprintf(stderr, "%s: cannot open\n", argv[1]);
    return 2;
  }
  char line[256];
  long n = 0;
  while (fgets(line, sizeof line, fh)) {
    ++n;
    int a[7];
    unsigned long long bits;
    if (sscanf(line, "Q %llx", &bits) == 1) {
      double v;
      memcpy(&v, &bits, sizeof v);
      const bool guard = overlay_cover::beyond_guard(v);
      printf("%d %d\n", guard ? 1 : 0, guard ? 0 : overlay_cover::quantise(v));
    } else if (sscanf(line, "S %d %d %d %d %d %d %d", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6) == 7) {
      printf("%d\n", overlay_cover::segment_covers(a[0], a[1], a[2], a[3], a[4], a[5], a[6]) ? 1 : 0);
    } else if (sscanf(line, "D %d %d %d %d %d", a, a + 1, a + 2, a + 3, a + 4) == 5) {
      printf("%d\n", overlay_cover::disc_covers(a[0], a[1], a[2], a[3], a[4]) ? 1 : 0);
    } else if (sscanf(line, "C %d %d %d", a, a + 1, a + 2) == 3) {
      int p0, p1;
      overlay_cover::centre_span(a[0], a[1], a[2], p0, p1);
      printf("%d %d\n", p0, p1);
    } else {
      fprintf(stderr, "%s:%ld: not a case: %s", argv[1], n, line);
      fclose(fh);
      return 2;
    }
  }
  fclose(fh);
  return 0;
}
