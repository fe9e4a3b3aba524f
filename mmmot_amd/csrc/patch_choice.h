// Which instantiation of the trunk's patch kernel serves a layer, and on how many workgroups: one pure host function, no
// HIP dependency, so that a test can ask it without a GPU (tests/test_patch_choice_cpu.py).  The four dispatchers of
// conv3x3_hl16_patch.hip (mmmot_conv3x3_bn_relu_hl16_patch, mmmot_conv3x3_raw_hl16, mmmot_conv3x3_bn_relu_hq8 and the
// fused first launches) and mmmot_patch_choice ask it; they have checked the arguments before (L, H, W >= 1,
// Cout % 64 == 0).
#pragma once

struct mmmot_patch_plan {
  int bn;     // output channels per tile: 64 or 128
  int bs;     // block edge: 16 (16 x 16 x 1 block per tile), 8 (8 x 8 x 4) or 4 (whole maps of at most 4 x 4, x 16)
  int items;  // tiles of the launch: pixel tiles x channel tiles
  int grid;   // workgroups of the persistent grid (0: no device - the launch is refused)
};

// block edge of a layer: 16 x 16 blocks unless the whole map fits an 8 x 8 block; maps of at most 4 x 4 pixels
// (conv5 at 64-pixel crops) take the halo-free whole-map geometry, 16 maps per tile.  min_block: the knob
// mmmot_set_patch_min_block (0 / 4 = automatic, 8 = no whole-map geometry).
static inline int mmmot_patch_block_edge(int H, int W, int min_block) {
  if (H > 8 || W > 8) return 16;
  if (H <= 4 && W <= 4 && min_block != 8) return 4;
  return 8;
}

// 128- or 64-channel tiles?  128 halves the LDS traffic per MFMA, but a small problem (one reference-shaped frame pair:
// 22 crops, 14 x 14 maps at conv5 = 88 tiles of 128 channels on 256 CUs) fills the chip better with twice as many
// 64-channel tiles.  Same arithmetic per output element either way (bitwise identical results).
static inline bool mmmot_patch_use_bn64(int L, int H, int W, int Cout, int n_cu, int min_block) {
  if (Cout % 128 != 0) return true;
  if (n_cu <= 0) return false;
  const int bs = mmmot_patch_block_edge(H, W, min_block), nb = 256 / (bs * bs);
  const long nblk = (long)L * ((H + bs - 1) / bs) * ((W + bs - 1) / bs);
  const long i128 = ((nblk + nb - 1) / nb) * (Cout / 128), i64 = 2 * i128;
  auto eff = [&](long items) { return (double)items / (double)(((items + n_cu - 1) / n_cu) * n_cu); };
  return 0.85 * eff(i64) > eff(i128);  // a 64-channel tile does half the work of a 128-channel one in ~0.59 of the time
}

// persistent grid: one workgroup per CU in whole XCDs (multiples of 8), capped by the knob mmmot_set_patch_grid_limit
// (0 = no cap) and by the items rounded up to 8
static inline int mmmot_patch_grid(int items, int n_cu, int grid_limit) {
  if (n_cu <= 0) return 0;
  int grid = (n_cu / 8) * 8;
  if (grid_limit > 0 && grid > grid_limit) grid = grid_limit;
  if (grid > ((items + 7) / 8) * 8) grid = ((items + 7) / 8) * 8;
  return grid;
}

// tiles of a launch with bn-channel tiles and bs x bs blocks
static inline int mmmot_patch_items(int L, int H, int W, int Cout, int bn, int bs) {
  const int nblk = L * ((H + bs - 1) / bs) * ((W + bs - 1) / bs), nb = 256 / (bs * bs);
  return ((nblk + nb - 1) / nb) * (Cout / bn);
}

// force_bn: the knob mmmot_set_patch_tile_width - 0 = the heuristic above, 64 = 64-channel tiles, 128 = 128-channel
// tiles wherever the layer has them (Cout % 128 == 0).  Results do not depend on it, bit for bit.
static inline mmmot_patch_plan mmmot_patch_choose(int L, int H, int W, int Cout, int n_cu, int min_block, int grid_limit,
                                                  int force_bn) {
  mmmot_patch_plan p;
  p.bs = mmmot_patch_block_edge(H, W, min_block);
  if (Cout % 128 != 0 || force_bn == 64) p.bn = 64;
  else if (force_bn == 128) p.bn = 128;
  else p.bn = mmmot_patch_use_bn64(L, H, W, Cout, n_cu, min_block) ? 64 : 128;
  p.items = mmmot_patch_items(L, H, W, Cout, p.bn, p.bs);
  p.grid = mmmot_patch_grid(p.items, n_cu, grid_limit);
  return p;
}

// Does the layer run in the M16 form (v_mfma_f32_16x16x32_f16 on fragment pairs exchanged in registers, see
// patch_fragments.inc)?  A property of the LAYER - its channel counts and its arithmetic - and of nothing else: never of
// L, the map size, the grid or a knob.  The two MFMA shapes round differently (one 32-deep sum against two 16-deep
// ones), so every instantiation a layer can get (64- / 128-channel tiles, 16 x 16 / 8 x 8 / whole-map blocks, pooled,
// unpooled, raw) must be of one form, or batched == alone and the other bitwise guarantees would break.
// The M16 K loop alternates two register assignments from stage to stage and starts every tile with the first one, so it
// needs an even number of stages per tile: Cin % 64 == 0.  The hq8 arithmetic and the fused first launch have no M16 form.
// Which layers: the ones measured faster by more than twice the run-to-run spread of the 32x32x16 form (DESIGN.md, section 7;
// profiles/m16) AND inside the 2e-6 bound the project holds a layer's output to: Cin = 128 .. 256 except 128 -> 128, whose
// gain stayed inside that spread.  The Cin = 64 launches are not power-limited and gain nothing; at Cin = 512 (K = 4608) the
// form is the fastest of all but its worst element measured 2.05e-6 of the output's maximum (tests/test_conv_patch_gpu.py).
static inline bool mmmot_patch_m16(int Cin, int Cout, int q8, int fused) {
  if (q8 || fused) return false;
  if (Cin == 128 && Cout == 128) return false;
  return Cin >= 128 && Cin <= 256 && Cin % 64 == 0;
}

// the fused first launches (conv1_1 + conv1_2 + pool): 64 channels, 16 x 16 blocks - no choice but the grid
static inline mmmot_patch_plan mmmot_patch_choose_fused(int L, int H, int W, int n_cu, int grid_limit) {
  mmmot_patch_plan p;
  p.bn = 64;
  p.bs = 16;
  p.items = mmmot_patch_items(L, H, W, 64, 64, 16);
  p.grid = mmmot_patch_grid(p.items, n_cu, grid_limit);
  return p;
}
