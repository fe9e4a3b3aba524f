// Stand-alone host program for tests/test_patch_choice_cpu.py: asks mmmot_patch_choose (csrc/patch_choice.h), the one
// function that picks the instantiation and the grid of a patch-kernel launch, for each case of a text file.
//   line in : L H W Cout n_cu min_block grid_limit force_bn     (Cout = 0: a fused first launch)
//   line out: bn bs items grid
#include <cstdio>

#include "../../mmmot_amd/csrc/patch_choice.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  int L, H, W, Cout, n_cu, min_block, grid_limit, force_bn;
  while (fscanf(f, "%d %d %d %d %d %d %d %d", &L, &H, &W, &Cout, &n_cu, &min_block, &grid_limit, &force_bn) == 8) {
    const mmmot_patch_plan p = Cout ? mmmot_patch_choose(L, H, W, Cout, n_cu, min_block, grid_limit, force_bn)
                                    : mmmot_patch_choose_fused(L, H, W, n_cu, grid_limit);
    if (Cout && p.bs != mmmot_patch_block_edge(H, W, min_block)) return 3;
    printf("%d %d %d %d\n", p.bn, p.bs, p.items, p.grid);
  }
  fclose(f);
  return 0;
}
