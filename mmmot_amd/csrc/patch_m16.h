// M16 form of the trunk's patch kernel (conv3x3_hl16_patch.hip): where an accumulator element of a 16x16x32 sub-tile
// lies in the 32-row x 32-channel product it belongs to, and where the epilogue stages it.  Pure integer functions, no
// HIP dependency, so that a test can compile them without a GPU (tests/test_m16_layout_cpu.py).
//
// A 32 x 32 product of the 32x32x16 form is four 16 x 16 sub-tiles (si, sj): rows 16 si .. + 15, channels 16 sj .. + 15.
// v_mfma_f32_16x16x32_f16 leaves element r (0..3) of lane l at row 4 (l / 16) + r, column l % 16 of its sub-tile.
#pragma once

#ifdef __HIPCC__
#define MM_M16_FN __host__ __device__ static inline constexpr
#else
#define MM_M16_FN static inline constexpr
#endif

// row (0..31) inside the 32-row block: four consecutive rows = the four registers of a lane = one 2 x 2 pooling window
MM_M16_FN int mm_m16_row(int si, int lane, int r) { return 16 * si + 4 * ((lane >> 4) & 3) + r; }
// channel (0..31) inside the 32-channel block
MM_M16_FN int mm_m16_col(int sj, int lane) { return 16 * sj + (lane & 15); }
// pooling quad (0..7) of the 32-row block a lane holds in sub-tile row si
MM_M16_FN int mm_m16_quad(int si, int lane) { return 4 * si + ((lane >> 4) & 3); }

// Staging rows.  Row stride of the fp32 staging area = BN + 4 floats = 4 banks (mod 32); a ds_write_b32 is served in two
// groups of 32 lanes = two 16-lane rows of the sub-tile each.
//  * unpooled: the two 16-lane rows of a group write rows 4 apart (4 x 4 = 16 banks apart): the natural row order is
//    conflict-free, the staged row IS the row of the block.
//  * pooled: the two 16-lane rows of a group hold CONSECUTIVE quads, 4 banks apart - a 12-lane overlap.  Quad q of the
//    block is therefore staged at slot mm_m16_pool_slot(q) (a permutation of 0..7 that puts them 4 slots apart) and the
//    store loop maps the slot it reads back to the quad (mm_m16_pool_quad).
MM_M16_FN int mm_m16_pool_slot(int q) { return 4 * (q & 1) + 2 * ((q >> 1) & 1) + ((q >> 2) & 1); }
MM_M16_FN int mm_m16_pool_quad(int slot) { return 4 * (slot & 1) + 2 * ((slot >> 1) & 1) + ((slot >> 2) & 1); }
