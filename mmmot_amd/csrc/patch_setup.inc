// conv3x3_hl16_patch_kernel, part 1 of 6 (textual part of the kernel body: the kernel is ONE function - its parts
// share ~60 locals and lambdas - cut where its phases begin so that each can be read on its own).
// Once per workgroup: tile shape constants, the LDS map, the conv1_1 weight fragments of the fused first layer, the
// XCD-aware item order (decode_item), the raw-window fetch of the fused first layer (fetch_raw), the block geometry
// of a tile and its per-thread patch source offsets (tile_blocks / poff_round / compute_poff), stream state.
  static_assert(!FUSE1 || (BN == 64 && BS == 16), "the fused first layer exists for 64-channel 16x16 tiles");
  static_assert(!RAW || (!POOL && !FUSE1 && !Q8), "raw fp32 output: plain unpooled f16x3 layers");
  static_assert(!M16 || (!FUSE1 && !Q8), "16x16x32 form: plain f16x3 layers");
  using G = PatchGeom<BS>;
  constexpr int WN = (BN == 128) ? 2 : 1;  // waves along channels
  constexpr int WM = 8 / WN;               // waves along pixels
  constexpr int TM = P_BM / (WM * 32);     // 2 / 1
  constexpr int TN = BN / (WN * 32);       // 2
  constexpr int B_BYTES = BN * P_ROWB;     // 16 / 8 KB per (tap, slab) weight tile
  constexpr int NBL = BN / 64;             // weight DMA instructions per wave per stage: 2 / 1
  constexpr int CLD = BN + 4;
  // LDS map: [patch buffer 0 | patch buffer 1 | weight ring (3 slots) | FUSE1: raw window].  The K loop is ONE
  // stream across the tiles of a workgroup: during the last slab of a tile the first patch slab of the NEXT tile
  // is fetched into the free patch buffer and the ring continues with the next tile's weight stages 0..2
  // ("transition" slab), so a tile has no load prologue.  (A CU pulls only ~5-8 B/clk from HBM - latency x
  // outstanding misses - so the 41 KB first slab plus three weight stages cost 15-20 k cycles when nothing runs
  // beside them: tools/patch_phase_timers.py.)  The epilogue therefore stages the accumulators through the
  // patch buffer the K loop has just finished with, in NCH row chunks, and leaves the other buffer and the ring
  // alone.  FUSE1 computes its patches (both buffers live all along): no transition, staging from offset 0.
  constexpr int P0_OFF = 0;
  constexpr int P1_OFF = G::BYTES;
  constexpr int RING0 = 2 * G::BYTES;
  constexpr int LOOP_BYTES = RING0 + 3 * B_BYTES;
  constexpr int RAW_OFF = LOOP_BYTES;                      // FUSE1: raw input window [3][20][20] fp32
  constexpr int RAW_BYTES = FUSE1 ? 3 * 20 * 20 * 4 + 64 : 0;
  constexpr bool OVL = FUSE1 && !Q8;                       // conv1_1 of the next tile under this tile's K loop (below)
  // pooled layers take the 2x2 maximum in registers (the four pixels of a window are four consecutive accumulator
  // registers of one lane: quad-ordered rows) and stage the 64 pooled rows only - one chunk
  constexpr int SROWS = POOL ? P_BM / 4 : P_BM;            // staged rows per tile
  constexpr int NCH = (FUSE1 || POOL) ? 1 : (SROWS / 2 * CLD * 4 <= G::BYTES) ? 2 : 4;
  constexpr int RCH = SROWS / NCH;                         // staged rows per epilogue chunk
  static_assert((FUSE1 && !OVL) ? (SROWS * CLD * 4 <= LOOP_BYTES) : (RCH * CLD * 4 <= G::BYTES), "epilogue staging does not fit");
  // STREAM: tiles are chained through transition slabs.  The successor's patch source table is made during the
  // tile's own prologue (low register pressure) and parked in LDS: [PA][512] words behind the ring.  The 8x8-block
  // variants have no room for it: they chain only onto a successor with the same pixel tile (same table).
  constexpr bool STREAM = !FUSE1 && (G::NB == 1 || G::WHOLE);
  // OVL (the f16x3 fused first layer): the conv1_1 patches of the NEXT tile are computed underneath the K loop of the
  // current one.  A third patch buffer makes that possible: a tile reads (X, Y) = its two 32-channel slabs; while its
  // second slab runs, the successor's first slab is written to Z and its second one to X (dead by then); the
  // epilogue stages through Y; the successor then works on (Z, X) with Y as its third buffer.  The prologue's VALU
  // work (conversions, ReLU, hi/lo split: ~150 instructions per 16-pixel round and wave, 3 rounds per wave and tile)
  // is cut into MFMA-slot-sized slices and issued in the shadow of the main loop's matrix instructions.
  constexpr int P2_OFF = (LOOP_BYTES + RAW_BYTES + 255) / 256 * 256;
  constexpr int POFF_OFF = OVL ? P2_OFF + G::BYTES : LOOP_BYTES + RAW_BYTES;
  // FUSE1: conv1_1 weights as MFMA A fragments [mb][lane][hi | lo] (8 KB) - read per use, not held in 32 registers
  constexpr int W1_OFF = POFF_OFF;
  // WHOLE: 256 zero bytes (one bank row) that stand in for every pixel outside the block
  constexpr int ZOFF = POFF_OFF + (STREAM ? G::PA * 512 * 4 : 0) + (FUSE1 ? 8192 : 0);
  static_assert(ZOFF % 256 == 0, "zero page: one aligned bank row");
  constexpr int SMEM = ZOFF + (G::WHOLE ? 256 : 0);
  static_assert(SMEM <= 160 * 1024, "LDS budget");
  __shared__ __attribute__((aligned(1024))) unsigned char smem[SMEM];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: LDS-DMA destinations stay in SGPRs
  if constexpr (G::WHOLE) {  // ordered before the first fragment read by the prologue barrier of the first tile
    if (tid < 16) reinterpret_cast<u32x4*>(smem + ZOFF)[tid] = u32x4{0u, 0u, 0u, 0u};
  }

  // Persistent workgroups: gridDim.x (a multiple of 8, at most one workgroup per CU - LDS allows no more)
  // workgroups walk the nitems = ntm * ntn tiles.  The dispatcher places workgroup b on XCD b % 8; every XCD
  // owns a contiguous chunk of the logical tile order (channel-tile-major inside the chunk, so the weights
  // of a channel tile stay in that XCD's L2) and its workgroups take the chunk's tiles round-robin.  One
  // launch-time workgroup per tile would leave the CU idle for a dispatch latency between tiles: with a
  // single resident workgroup nothing overlaps it (measured: fixed cost of ~2 channel slabs per tile).
  // FUSE1: conv1_1 weight fragments (A operand of v_mfma_f32_16x16x32_f16: channel 16 mb + (lane & 15),
  // k = 8 (lane >> 4) .. + 7 - the whole K = 32 in one step) are staged in LDS once per workgroup ([W1_OFF]; read per
  // use by the serial form; the overlapped form (OVL) keeps them in 32 registers - the K loop of this layer is bound by
  // LDS reads, one per MFMA).  The folded bias / 2^-shift rides in the k = 27 slot of the K = 32 step (27 taps x colours
  // padded to 32): its "window value" is the constant 1, so the matrix cores add it - no fma and no bias read in the
  // epilogue of a round; hi + lo keep 22 bits of it like of every weight (|bias| / 2^-shift must stay below 65504:
  // pack.conv1_weight_shift).  The raw-window offsets of the 8 k values a lane gathers are fixed (k >= 28: offset 0 -
  // the weight is zero and the window value finite, so the gather needs no branch)
  int roff[8];
  f16x8 w1h[4], w1l[4];  // OVL only
  if constexpr (FUSE1) {
    const int kg1 = (threadIdx.x & 63) >> 4;
    {
      const int t = threadIdx.x;
      const int mb = t >> 7, ln = (t >> 1) & 63, hl = t & 1;
      u32x4 wv = fz.w1[((mb * 16 + (ln & 15)) * 4 + (ln >> 4)) * 2 + hl];
      if ((ln >> 4) == 3) {  // k = 24 .. 31 of this channel: element 3 = k 27 takes the bias (the window value there is 1)
        const float bs = fz.bias1[mb * 16 + (ln & 15)] * (1.f / fz.oscale1);  // oscale1 is a power of two
        const _Float16 bh = (_Float16)bs;
        const _Float16 bl = mm_hl_lo(bs, bh);
        const unsigned bits = (unsigned)__builtin_bit_cast(unsigned short, hl == 0 ? bh : bl);
        wv[1] = (wv[1] & 0x0000ffffu) | (bits << 16);
      }
      reinterpret_cast<u32x4*>(smem + W1_OFF)[t] = wv;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = 8 * kg1 + e;
      const int tap = k / 3, c = k - 3 * tap;
      roff[e] = (k < 27) ? c * 400 + (tap / 3) * 20 + (tap % 3) : 0;
    }
  }
  const int nitems = ntm * ntn;
  const int xq = nitems >> 3, xr = nitems & 7;
  const int xcd = blockIdx.x & 7;
  const int cbase = (xcd < xr) ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq;
  const int clen = (xcd < xr) ? xq + 1 : xq;
  auto decode_item = [&](int item, int& mt, int& nt) {
    if (clen % ntn == 0 && cbase % ntn == 0) {
      const int mcount = clen / ntn;
      nt = item / mcount;
      mt = cbase / ntn + item % mcount;
    } else {
      mt = (cbase + item) / ntn;
      nt = (cbase + item) % ntn;
    }
  };
  // FUSE1: the raw input window of the NEXT tile is fetched into registers while the current tile's
  // epilogue runs (nothing else hides that round trip: one workgroup per CU)
  // The three window values of a thread are REQUESTED by fetch_raw and turned into what conv1_1 reads (zero outside the
  // image; 8-bit crops: ToTensor + Normalize) only where they are consumed (raw_value): a select or a conversion right
  // behind the load makes the compiler wait for it on the spot - with vmcnt(0), in the middle of the K loop, draining
  // the weight ring's requests with it (round 6: one memory round trip per tile for fp32 crops, three chained ones for
  // 8-bit crops, in every wave).
  // (whether an element lies inside the image is recomputed at the consumption point from the tile index instead of
  // being carried in a register across the K loop: the overlapped form has none to spare)
  float rawv[3] = {0.f, 0.f, 0.f};   // fp32 crops: the value; 8-bit crops: the byte (as an integer bit pattern)
  bool raw_ready = false;
  auto raw_inside = [&](int mtile, int k, int& c, int& crop, int& gy, int& gx) -> bool {
    const int nbpc_ = nby * nbx;
    crop = mtile / nbpc_;
    const int br = mtile - crop * nbpc_;
    const int by = br / nbx, bx = br - by * nbx;
    // (laundered like the lane id of poff_round: otherwise the thread-only parts of the three addresses are hoisted out
    // of the tile loop, stay live across the K loop and are spilled - with a vmcnt(0) in front of every reload)
    int tid_ = threadIdx.x;
    asm volatile("" : "+v"(tid_));
    const int i = tid_ + 512 * k;
    c = i / 400;
    const int rem = i - c * 400;
    const int wy = rem / 20, wx = rem - wy * 20;
    gy = by * 16 - 2 + wy;
    gx = bx * 16 - 2 + wx;
    return i < 1200 && mtile < nblk && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
  };
  auto fetch_raw = [&](int mtile) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      int c, crop, gy, gx;
      // every wave issues exactly one load per k (invalid lanes read element 0): the counted vmcnt waits of the
      // overlapped prologue rely on the number of loads in flight
      const bool ok = raw_inside(mtile, k, c, crop, gy, gx);
      if (fz.raw8) {
        const long idx = ok ? (((long)crop * H + gy) * W + gx) * 3 + c : 0;
        rawv[k] = __builtin_bit_cast(float, (unsigned)fz.raw8[idx]);
      } else {
        const long idx = ok ? (((long)crop * 3 + c) * H + gy) * W + gx : 0;
        rawv[k] = fz.raw[idx];
      }
    }
  };
  auto raw_value = [&](int mtile, int k) -> float {  // window element k (of tile mtile) of this thread as conv1_1 reads it
    int c, crop, gy, gx;
    const bool ok = raw_inside(mtile, k, c, crop, gy, gx);
    float v = rawv[k];
    if (fz.raw8) {
      // (selects, not fz.mean[c]: a runtime index into the kernel-argument struct is a global load with its own wait)
      const float mu = c == 0 ? fz.mean[0] : (c == 1 ? fz.mean[1] : fz.mean[2]);
      const float sd = c == 0 ? fz.stdv[0] : (c == 1 ? fz.stdv[1] : fz.stdv[2]);
      const float x = __fdiv_rn((float)__builtin_bit_cast(unsigned, v), 255.f);   // ToTensor
      v = __fdiv_rn(__fsub_rn(x, mu), sd);                                        // Normalize
    }
    return ok ? v : 0.f;
  };
  // patch source offsets of one tile (16-byte units, without the slab term; ~0u = zero page).  Round k moves pieces
  // [k*512 + wave*64, +64) (k < FULL) or, in the partial round, [FULL*512 + wave*RL, +RL); piece p = (patch pixel
  // n = p >> 3, LDS slot c' = p & 7) holds the logical piece c' ^ swz_a(py, px) of that pixel's 128-byte slab
  // record.  The block -> (crop, by, bx) divisions are wave-uniform (scalar unit); the table of the NEXT tile is
  // computed while the slower waves still issue their stores, ahead of the closing barrier of the tile.
  unsigned poff[G::PA];
  struct TileBlocks {
    int crop[G::NTB], gy0[G::NTB], gx0[G::NTB];  // wave-uniform: crop (-1: no such block) and patch origin of each block
  };
  auto tile_blocks = [&](int mtile, TileBlocks& tb) {
    if constexpr (G::WHOLE) {  // block q of the tile = crop mtile * NB + q, origin (0, 0), no halo
      tb.crop[0] = mtile * G::NB;
      tb.gy0[0] = 0;
      tb.gx0[0] = 0;
      return;
    }
    const int nbpc_ = nby * nbx;
#pragma unroll
    for (int q = 0; q < G::NTB; ++q) {
      const int b = mtile * G::NB + q;
      const int crop = b / nbpc_, br = b - crop * nbpc_;
      const int by = br / nbx;
      tb.crop[q] = (b < nblk) ? crop : -1;
      tb.gy0[q] = by * BS - 1;
      tb.gx0[q] = (br - by * nbx) * BS - 1;
    }
  };
  auto poff_round = [&](auto KC, const TileBlocks& tb) -> unsigned {
    constexpr int k = decltype(KC)::value;
    const int cin16 = (Cin >> 3) * 2;
    // the lane id is laundered: otherwise the lane-only part of every round (pixel, swizzle) is hoisted out of
    // the tile loop and stays live across the K loop (+20 VGPRs at its register peak)
    int lane_ = lane;
    asm volatile("" : "+v"(lane_));
    const int p = (k < G::FULL) ? (k * 8 + wave) * 64 + lane_ : G::FULL * 512 + wave * G::RL + lane_;
    unsigned off = ~0u;
    if (k < G::FULL || lane_ < G::RL) {
      const int n = p >> 3, c = p & 7;
      const int blk = n / G::PP;
      const int rem = n - blk * G::PP;
      const int py = rem / G::PW, px = rem - py * G::PW;
      int crop = tb.crop[0], gy = tb.gy0[0] + py, gx = tb.gx0[0] + px;
      if constexpr (G::WHOLE) {
        crop += blk;
        if (crop >= nblk) crop = -1;
      }
#pragma unroll
      for (int q = 1; q < G::NTB; ++q)
        if (blk == q) {
          crop = tb.crop[q];
          gy = tb.gy0[q] + py;
          gx = tb.gx0[q] + px;
        }
      int swz;
      if constexpr (G::WHOLE) swz = pt_swz_w<BS>(blk, py);
      else swz = pt_swz_a(py, px);
      if (crop >= 0 && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W)
        off = (unsigned)(((crop * H + gy) * W + gx) * cin16 + (c ^ swz));
    }
    return off;
  };
  auto compute_poff = [&](int mtile) {
    TileBlocks tb;
    tile_blocks(mtile, tb);
    poff[0] = poff_round(std::integral_constant<int, 0>{}, tb);
    poff[1] = poff_round(std::integral_constant<int, 1>{}, tb);
    poff[2] = poff_round(std::integral_constant<int, 2>{}, tb);
    poff[3] = poff_round(std::integral_constant<int, 3>{}, tb);
    if constexpr (G::PA > 4) poff[4] = poff_round(std::integral_constant<int, 4>{}, tb);
    if constexpr (G::PA > 5) poff[5] = poff_round(std::integral_constant<int, 5>{}, tb);
    if constexpr (G::PA > 6) poff[6] = poff_round(std::integral_constant<int, 6>{}, tb);
  };
  int mt = 0, nt = 0;
  if ((int)(blockIdx.x >> 3) < clen) {
    decode_item(blockIdx.x >> 3, mt, nt);
    if constexpr (!FUSE1) compute_poff(mt);
  }
  const u32x4* wbase = wp + (long)(nt * BN) * ((Cin >> 3) * 2);  // weight rows of this tile's channel tile
  const u32x4* wbase_next = wbase;
  bool primed = false;  // this tile's patch slab 0 and weight stages 0..2 were streamed in by the previous tile
  int pcur = P0_OFF;    // patch buffer of the current slab (byte offset in smem)
  int pnext = P1_OFF;   // patch buffer being filled for the next slab (of this tile or the next one)
  int bufX = P0_OFF, bufY = P1_OFF, bufZ = OVL ? P2_OFF : 0;  // OVL: this tile's two slabs and the free buffer
