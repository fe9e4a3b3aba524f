// Host program of tests/test_m16_layout_cpu.py: prints the epilogue index functions of the M16 form (csrc/patch_m16.h)
// and the per-layer rule (csrc/patch_choice.h), both compiled without HIP.
//   index            -> one line per (si, sj, lane, r): row col quad slot(quad) quad(slot(quad))
//   rule <file>      -> per line "Cin Cout q8 fused" of the file: 0 / 1
#include <cstdio>
#include <cstring>

#include "../../mmmot_amd/csrc/patch_choice.h"
#include "../../mmmot_amd/csrc/patch_m16.h"

int main(int argc, char** argv) {
  if (argc >= 2 && !std::strcmp(argv[1], "index")) {
    for (int si = 0; si < 2; ++si)
      for (int sj = 0; sj < 2; ++sj)
        for (int lane = 0; lane < 64; ++lane)
          for (int r = 0; r < 4; ++r) {
            const int q = mm_m16_quad(si, lane), s = mm_m16_pool_slot(q);
            std::printf("%d %d %d %d %d\n", mm_m16_row(si, lane, r), mm_m16_col(sj, lane), q, s, mm_m16_pool_quad(s));
          }
    return 0;
  }
  if (argc >= 3 && !std::strcmp(argv[1], "rule")) {
    std::FILE* f = std::fopen(argv[2], "r");
    if (!f) return 2;
    int cin, cout, q8, fused;
    while (std::fscanf(f, "%d %d %d %d", &cin, &cout, &q8, &fused) == 4)
      std::printf("%d\n", mmmot_patch_m16(cin, cout, q8, fused) ? 1 : 0);
    std::fclose(f);
    return 0;
  }
  return 1;
}
