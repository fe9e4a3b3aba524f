// Which kernel serves a call of mmmot_gemm_rows (include/mmmot_hip.h) - the wide kernel of gemm_wide.hip or the tile
// kernel of gemm_rows.hip - and with which launch geometry: one pure host function, no HIP dependency, so that a test can
// ask it without a GPU (tests/test_wide_choice_cpu.py).  mmmot_gemm_wide_try and gw_launch (gemm_wide.hip) and
// mmmot_gemm_rows_choice ask it; mmmot_gemm_rows has checked the arguments before.
#pragma once
#include "../../include/mmmot_hip.h"

struct mmmot_wide_plan {
  int wide;    // 1: the wide kernel takes the launch, 0: the tile kernel
  int nh;      // wide: row tiles of 128 rows per workgroup, 1 (four waves) | 2 (eight waves); tile kernel: 0
  int ntn;     // column tiles: N / 256 (wide), N / 128 or N / 64 (tile kernel)
  int nitems;  // wide: items of the launch, padded to whole groups of 8 * ntn; tile kernel: T * ntn
  int grid;    // workgroups: the persistent grid (wide), one per item (tile kernel)
};

// variant: mmmot_set_gemm_rows_variant - 0 = automatic, 1 = the tile kernel only, 3 / 4 = the wide kernel whenever the
// layer is eligible, with NH = 1 / NH = 2.  grid_limit: mmmot_set_gemm_wide_grid_limit - 0 = automatic, n > 0 caps the
// persistent grid at n, rounded down to whole groups of 8 * ntn and never below one group (the launcher's floor, the
// grid an 8-CU part launches).  Results do not depend on either, bit for bit.
static inline mmmot_wide_plan mmmot_wide_choose(const mmmot_gemm_args* a, int n_cu, int variant, int grid_limit) {
  mmmot_wide_plan p;
  p.wide = 0;
  p.nh = 0;
  p.ntn = a->N / (a->N % 128 == 0 ? 128 : 64);
  p.nitems = p.grid = a->T * p.ntn;
  if (variant == 1) return p;
  if (!a->w_hl16 || (a->K != 256 && a->K != 512) || a->N % 128 != 0) return p;  // (whole 256-value pieces of the uniform rows)
  if (a->amode != MMMOT_A_PAIR && a->amode != MMMOT_A_NORM_RELU) return p;
  if (a->dbias || a->colsum || a->act != MMMOT_ACT_NONE) return p;
  if (a->amode == MMMOT_A_PAIR && (a->ldf % 4 != 0 || a->K > a->ldf || !a->pair_uniform32)) return p;
  if (a->amode == MMMOT_A_NORM_RELU && a->ldsc < a->K) return p;
  if (a->Y && (a->ldy % 4 != 0)) return p;
  if (n_cu <= 0) return p;
  if (a->N % 256 != 0) return p;  // 256-column items (the N = 128 layer of the block is HBM-bound on the tile kernel)
  const long items = (long)((a->T + 1) / 2) * (a->N / 256);
  // small problems (one reference-shaped frame pair) are latency-bound: more, smaller workgroups finish sooner
  if (variant == 0 && items < n_cu / 2) return p;
  // eight waves sharing the weight stages win once every workgroup walks a long chain of items (cfg4's 32-pair batches:
  // -4 .. -6 % against the four-wave form, tools/bench_rows_gemm.py); below that the two forms are within the box spread
  // of each other and the four-wave form fills the chip with half as many rows
  const bool nh2 = (variant == 4) || (variant == 0 && items >= 24L * n_cu);
  p.wide = 1;
  p.nh = nh2 ? 2 : 1;
  p.ntn = a->N / 256;
  const int group = 8 * p.ntn;
  const int nu = (a->T + p.nh - 1) / p.nh;           // groups of NH row tiles
  p.nitems = ((nu + 7) / 8) * group;                 // padded to whole groups of 8 x ntn column tiles
  // NH = 1: two workgroups per CU; whole groups (column tiles of a row tile on one XCD)
  p.grid = ((2 / p.nh) * n_cu / group) * group;
  if (p.grid < group) p.grid = group;
  if (grid_limit > 0 && p.grid > grid_limit) p.grid = (grid_limit / group) * group;
  if (p.grid < group) p.grid = group;
  if (p.grid > p.nitems) p.grid = p.nitems;
  return p;
}
