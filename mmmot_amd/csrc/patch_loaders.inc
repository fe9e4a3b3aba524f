// conv3x3_hl16_patch_kernel, part 2 of 6.  Per item: accumulators, wave / lane roles, and the loaders - everything
// arrives by LDS-DMA: issue_patch_round (haloed activation patch of a 32-channel slab, swizzled on the source side),
// issue_b1 / issue_b (the (tap, slab) weight tile into the 3-slot ring), issue_tile_head (first patch slab + weight
// stages 0..2 of a tile that has no predecessor streaming them in).
  PT_STAMP_DECL()
  PT_STAMP(-1)
  const int n0 = nt * BN;
  const int cin8 = Cin >> 3;
  const int nslab = Cin >> 5;
  const int nbpc = nby * nbx;  // blocks per crop

  f32x16 acc[TM][TN];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[tm][tn][e] = 0.f;
  // M16: the same 32 x 32 products as four 16 x 16 sub-tiles [si][sj] each (patch_m16.h), `acc` stays unused
  f32x4 acc16[TM][TN][2][2];
  if constexpr (M16) {
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc16[tm][tn][s >> 1][s & 1] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int wm = wave / WN, wn = wave % WN;
  const int lr = lane & 31;
  const int h = lane >> 5;

  // ---------------- loader state ---------------------------------------------------------------------
  // patch: round k moves pieces [k*512 + wave*64, +64) (k < FULL) or, in the partial round,
  // [FULL*512 + wave*RL, +RL); piece p = (patch pixel n = p >> 3, LDS slot c' = p & 7) holds the
  // logical piece c' ^ swz_a(py, px) of that pixel's 128-byte slab record.
  const u32x4* zsrc = pt_zero_page + (lane & 15);
  // weights: instruction (wave * NBL + b) covers 8 rows of the tile; lane = (row in 8, slot in row)
  const int rsub = lane >> 3, slot8 = lane & 7;
  unsigned boffl[NBL];  // lane part of the weight source offset (16-byte units); the rest is wave-uniform
#pragma unroll
  for (int b = 0; b < NBL; ++b) {
    const int brw = (wave * NBL + b) * 8 + rsub;
    boffl[b] = (unsigned)(brw * (cin8 * 2) + (slot8 ^ pt_swz_b(brw)));
  }
  const long tapstride_w = (long)Cout * cin8 * 2;

  auto issue_patch_round = [&](auto KC, int slab, int pbuf) {  // pbuf: byte offset of the patch buffer in smem
    constexpr int k = decltype(KC)::value;
    const u32x4* src = (poff[k] != ~0u) ? in + (poff[k] + (unsigned)(slab * 8)) : zsrc;
    if constexpr (k < G::FULL) {
      mm_dma16(src, smem + pbuf + (k * 8 + wave) * 1024);
    } else {
      if (lane < G::RL) mm_dma16(src, smem + pbuf + G::FULL * 8192 + wave * (G::RL * 16));
    }
  };
  // weight DMA instruction b (0..NBL-1) of stage (tap, slab) into ring slot `ringslot`
  auto issue_b1 = [&](auto BC, const u32x4* base, int tap, int slab, int ringslot) {
    constexpr int b = decltype(BC)::value;
    if constexpr (b < NBL) {
      // wave-uniform base, laundered through readfirstlane so that it stays in scalar registers and is
      // not re-associated with the lane offsets into nine hoisted 64-bit lane values
      const unsigned long ubl = (unsigned long)(base + ((long)tap * tapstride_w + slab * 8));
      const unsigned ub_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(ubl >> 32));
      const unsigned ub_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)ubl);
      const u32x4* ub = (const u32x4*)(((unsigned long)ub_hi << 32) | (unsigned long)ub_lo);
      mm_dma16(ub + boffl[b], smem + RING0 + ringslot * B_BYTES + (wave * NBL + b) * 1024);
    }
  };
  auto issue_b = [&](int tap, int slab, int ringslot) {
    issue_b1(std::integral_constant<int, 0>{}, wbase, tap, slab, ringslot);
    issue_b1(std::integral_constant<int, 1>{}, wbase, tap, slab, ringslot);
  };
  // first tile of a workgroup: patch slab 0 -> buffer pbuf, weight stages 0..2 (poff / wbase are current)
  auto issue_tile_head = [&](int pbuf) {
    issue_patch_round(std::integral_constant<int, 0>{}, 0, pbuf);
    issue_patch_round(std::integral_constant<int, 1>{}, 0, pbuf);
    issue_patch_round(std::integral_constant<int, 2>{}, 0, pbuf);
    issue_patch_round(std::integral_constant<int, 3>{}, 0, pbuf);
    if constexpr (G::PA > 4) issue_patch_round(std::integral_constant<int, 4>{}, 0, pbuf);
    if constexpr (G::PA > 5) issue_patch_round(std::integral_constant<int, 5>{}, 0, pbuf);
    if constexpr (G::PA > 6) issue_patch_round(std::integral_constant<int, 6>{}, 0, pbuf);
    issue_b(0, 0, 0);
    issue_b(1, 0, 1);
    issue_b(2, 0, 2);
  };
