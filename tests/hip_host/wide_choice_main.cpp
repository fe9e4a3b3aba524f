// Stand-alone host program for tests/test_wide_choice_cpu.py: asks mmmot_wide_choose (csrc/wide_choice.h), the one
// function that decides between the wide and the tile kernel behind mmmot_gemm_rows and sets the wide launch's geometry,
// for each case of a text file.
//   line in : variant n_cu grid_limit T N K amode w_hl16 dbias colsum act ldf pair_uniform32 ldsc ldy Y
//             (dbias, colsum, Y: 0 = NULL, 1 = present)
//   line out: wide nh ntn nitems grid
#include <cstdio>

#include "../../include/mmmot_hip.h"
#include "../../mmmot_amd/csrc/wide_choice.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  static float some_rows[4] = {0.f, 0.f, 0.f, 0.f};  // the chooser asks whether a pointer is there, never reads it
  int variant, n_cu, limit, T, N, K, amode, w_hl16, dbias, colsum, act, ldf, uni, ldsc, ldy, y;
  while (fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &variant, &n_cu, &limit, &T, &N, &K, &amode, &w_hl16,
                &dbias, &colsum, &act, &ldf, &uni, &ldsc, &ldy, &y) == 16) {
    mmmot_gemm_args a = {};
    a.T = T;
    a.N = N;
    a.K = K;
    a.amode = amode;
    a.w_hl16 = w_hl16;
    a.dbias = dbias ? some_rows : nullptr;
    a.colsum = colsum ? some_rows : nullptr;
    a.act = act;
    a.ldf = ldf;
    a.pair_uniform32 = uni;
    a.ldsc = ldsc;
    a.ldy = ldy;
    a.Y = y ? some_rows : nullptr;
    const mmmot_wide_plan p = mmmot_wide_choose(&a, n_cu, variant, limit);
    printf("%d %d %d %d %d\n", p.wide, p.nh, p.ntn, p.nitems, p.grid);
  }
  fclose(f);
  return 0;
}
