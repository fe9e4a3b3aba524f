// conv3x3_hl16_patch_kernel, part 6 of 6.  Epilogue of a tile: accumulators -> LDS (fp32, quad-ordered rows; pooled
// layers take the 2 x 2 maximum in registers first) -> per-output-channel scale, bias, ReLU, range guard, encode (hl16
// split / hq8 record / raw fp32 rows) -> global stores; then the hand-over to the successor tile.
  if constexpr (FUSE1 && !OVL) {
    raw_ready = has_next;
    if (raw_ready) fetch_raw(mt_next);
  }
  // ---- epilogue: accumulators -> LDS fp32 [256][BN+4] -> pool/bias/relu/split -> hl16 -------------
  // thread -> fixed channel unit u (8 channels) and rows r0, r0 + RSTEP, ...: bias is loaded once, before
  // the barriers (a load inside the store loop costs one L2 round trip per iteration)
  constexpr int UN = BN / 8;
  constexpr int RSTEP = 512 / UN;  // 32 / 64
  const int eu = tid % UN, er0 = tid / UN;
  const f32x8 bv = *reinterpret_cast<const f32x8*>(&bias[n0 + eu * 8]);
  const f32x8 sv = *reinterpret_cast<const f32x8*>(&oscv[n0 + eu * 8]);  // per-output-channel 2^-shift
  // Q8: thread -> 16 channels (hi = two pieces, fp8 copies = one piece each: 4 stores of 16 bytes per 16 channels)
  constexpr int UN16 = BN / 16;
  constexpr int RSTEP16 = 512 / UN16;  // 64 / 128
  const int eu16 = tid % UN16, er16 = tid / UN16;
  float bq[16], sq[16];
  if constexpr (Q8) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      bq[e] = bias[n0 + eu16 * 16 + e];
      sq[e] = oscv[n0 + eu16 * 16 + e];
    }
  }
  // blocks of this tile: validity and first pixel (block-local (0,0)) of each
  int bcrop[G::NTB], bgy0[G::NTB], bgx0[G::NTB];
#pragma unroll
  for (int k = 0; k < G::NTB; ++k) {
    const int b = mt * G::NB + k;
    const int crop = b / nbpc;
    const int br = b - crop * nbpc;
    const int by = br / nbx;
    bcrop[k] = (b < nblk) ? crop : -1;
    bgy0[k] = by * BS;
    bgx0[k] = (br - by * nbx) * BS;
  }
  // pixel (y, x) of block blk of this tile -> crop (-1: no such block), image coordinates (WHOLE: the block is the
  // whole map of crop mt * NB + blk)
#define PT_BLK_PIXEL(blk, y, x)                                   \
  int crop = bcrop[0], gy = bgy0[0] + (y), gx = bgx0[0] + (x);    \
  if constexpr (G::WHOLE) {                                       \
    crop = mt * G::NB + (blk);                                    \
    if (crop >= nblk) crop = -1;                                  \
  } else {                                                        \
    _Pragma("unroll") for (int k = 1; k < G::NTB; ++k) if ((blk) == k) { \
      crop = bcrop[k];                                            \
      gy = bgy0[k] + (y);                                         \
      gx = bgx0[k] + (x);                                         \
    }                                                             \
  }
  {
  // barriers of the epilogue order LDS traffic only (lgkmcnt): a __syncthreads() would also drain vmcnt, i.e.
  // wait for the successor's loads and for this tile's own global stores
  mm_lds_barrier();  // every wave is past its last read of the buffer that becomes the staging area
  PT_STAMP(2)
  float* Cs = reinterpret_cast<float*>(smem + ((FUSE1 && !OVL) ? 0 : pcur));
  if constexpr (OVL) {
    if (rawfly) {  // every wave is past its gathers from the successor's window: the one after it moves in
      float* R = reinterpret_cast<float*>(smem + RAW_OFF);
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (tid + 512 * k < 1200) R[tid + 512 * k] = raw_value(mt_next2, k);
    }
  }
  const int cout8 = Cout >> 3;
  // the per-channel vectors are consumed HERE, outside the conditional store blocks: the compiler waits for their loads
  // once (they were issued in front of the barriers) - inside the blocks the same wait would be a vmcnt(0) behind the
  // previous block's global stores, i.e. a store round trip per block
  if constexpr (Q8) {
#pragma unroll
    for (int e = 0; e < 16; ++e) asm volatile("" ::"v"(bq[e]), "v"(sq[e]));
  } else {
    asm volatile("" ::"v"(bv), "v"(sv));
  }
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
  if (ch > 0) mm_lds_barrier();  // the previous chunk has been read by everyone
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) {
    const int rb = wm * TM + tm;  // 32-row block of the tile (wave-uniform)
    if constexpr (M16 && POOL) {
      // the four registers of a lane are rows 4 (l / 16) .. + 3 of its sub-tile = quad mm_m16_quad; the quads are staged in
      // the slot order of patch_m16.h (conflict-free writes), which the store loop below undoes
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const f32x4 c = acc16[tm][tn][s >> 1][s & 1];
          const float m = fmaxf(fmaxf(c[0], c[1]), fmaxf(c[2], c[3]));
          Cs[(rb * 8 + mm_m16_pool_slot(mm_m16_quad(s >> 1, lane))) * CLD + wn * TN * 32 + tn * 32 + mm_m16_col(s & 1, lane)] = m;
        }
    } else if constexpr (M16) {
      if (rb / (8 / NCH) == ch) {
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              Cs[((rb % (8 / NCH)) * 32 + mm_m16_row(s >> 1, lane, r)) * CLD + wn * TN * 32 + tn * 32 + mm_m16_col(s & 1, lane)] =
                  acc16[tm][tn][s >> 1][s & 1][r];
      }
    } else if constexpr (POOL) {
      // quad q = 2j + h of the 32-row block holds rows 8j + 4h .. + 3 = accumulator registers 4j .. 4j + 3
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float m = fmaxf(fmaxf(acc[tm][tn][4 * j], acc[tm][tn][4 * j + 1]),
                                fmaxf(acc[tm][tn][4 * j + 2], acc[tm][tn][4 * j + 3]));
          Cs[(rb * 8 + 2 * j + h) * CLD + wn * TN * 32 + tn * 32 + lr] = m;
        }
    } else if (rb / (8 / NCH) == ch) {
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int e = 0; e < 16; ++e)
          Cs[((rb % (8 / NCH)) * 32 + mm_acc_row(e, lane)) * CLD + wn * TN * 32 + tn * 32 + lr] = acc[tm][tn][e];
    }
  }
  mm_lds_barrier();
  if (ch == 0) { PT_STAMP(3) }
  // The staged values are read with mm_lds_read32 / mm_lds_wait (common.h).  The compiler cannot tell the staging buffer
  // from the LDS-DMA destinations of the successor tile (both are runtime offsets into one array), so it answers every LDS
  // read it can see with s_waitcnt vmcnt(0) - and vmcnt also counts this tile's own global STORES: each iteration of the
  // store loop then waited for the previous iteration's stores to reach the L2 (8 round trips per unpooled tile, ~10 % of
  // the tile: the "encode + issue stores" phase of profiles/HISTORY.md).  The buffer really is disjoint from everything
  // in flight (patch_setup.inc).
  if constexpr (Q8) {
    const int Hq = H >> 1, Wq = W >> 1;
    constexpr int NITEM = RCH;  // quads (pooled) or rows of one chunk
    constexpr int NIT16 = (NITEM + RSTEP16 - 1) / RSTEP16;
    f32x4 vq[NIT16][4];  // 16 staged values per item, requested before the first store
#pragma unroll
    for (int i = 0; i < NIT16; ++i) {
      const int itl = er16 + i * RSTEP16;
      const unsigned ad = mm_lds_addr(&Cs[(itl < NITEM ? itl : 0) * CLD + eu16 * 16]);
      mm_lds_read32(ad, vq[i][0], vq[i][1]);
      mm_lds_read32(ad + 32, vq[i][2], vq[i][3]);
    }
    mm_lds_wait();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < NIT16; ++i) {
      const int itl = er16 + i * RSTEP16;  // chunk-local
      const int it = ch * NITEM + itl;
      if (itl < NITEM) {
        int blk, y, x;
        if constexpr (POOL) pt_row_to_pixel<BS>(it >> 3, (it & 7) * 4, blk, y, x);
        else pt_row_to_pixel<BS>(it >> 5, it & 31, blk, y, x);
        PT_BLK_PIXEL(blk, y, x)
        // pooled layers floor odd maps like nn.MaxPool2d(2, 2) (reference modules/vgg.py:72): a window that sticks out
        // of the image (last row / column of an odd map) produces no output
        if (crop >= 0 && gy < H && gx < W && (!POOL || ((gy >> 1) < Hq && (gx >> 1) < Wq))) {
          float v[16];
#pragma unroll
          for (int e = 0; e < 16; e += 4) {
            const f32x4 w4 = vq[i][e >> 2];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[e + k] = fmaxf(fmaf(w4[k], sq[e + k], bq[e + k]), 0.f);
          }
          pt_range_guard<16>(v, true, rng);
          u32x4 hi0, hi1, a8, l8;
          pt_encode_q8(v, hi0, hi1, a8, l8);
          const long pix = POOL ? ((long)crop * Hq + (gy >> 1)) * Wq + (gx >> 1) : ((long)crop * H + gy) * W + gx;
          const int c0 = n0 + eu16 * 16;  // first channel: 32-channel block c0 >> 5, 16-channel half (c0 >> 4) & 1
          u32x4* o = out + (pix * cout8 * 2) + (c0 >> 5) * 8;
          const int hf = (c0 >> 4) & 1;
          if constexpr (!POOL) {
            // unpooled layers write 131 KB per tile that nothing re-reads before it has left the caches (a layer's
            // output is 1-2 GB per step): streaming stores, -3 % on the 512-channel layers, neutral elsewhere
            __builtin_nontemporal_store(hi0, &o[2 * hf]);
            __builtin_nontemporal_store(hi1, &o[2 * hf + 1]);
            __builtin_nontemporal_store(a8, &o[4 + hf]);
            __builtin_nontemporal_store(l8, &o[6 + hf]);
          } else {
            o[2 * hf] = hi0;
            o[2 * hf + 1] = hi1;
            o[4 + hf] = a8;
            o[6 + hf] = l8;
          }
        }
      }
    }
  } else if constexpr (POOL) {
    const int Hq = H >> 1, Wq = W >> 1;
    constexpr int NQ = RCH;  // quads of the (single) chunk
    constexpr int NIT = (NQ + RSTEP - 1) / RSTEP;
    f32x4 va[NIT], vb[NIT];  // requested before the first store
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int qdl = er0 + i * RSTEP;
      mm_lds_read32(mm_lds_addr(&Cs[(qdl < NQ ? qdl : 0) * CLD + eu * 8]), va[i], vb[i]);
    }
    mm_lds_wait();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int qdl = er0 + i * RSTEP;  // chunk-local
      const int qd = ch * NQ + qdl;
      if (qdl >= NQ) continue;
      int blk, y, x;
      pt_row_to_pixel<BS>(qd >> 3, (M16 ? mm_m16_pool_quad(qd & 7) : (qd & 7)) * 4, blk, y, x);  // M16: staged slot -> quad
      PT_BLK_PIXEL(blk, y, x)
      if (crop >= 0 && gy < H && gx < W && (gy >> 1) < Hq && (gx >> 1) < Wq) {  // floor pooling: see the hq8 branch
        f32x8 v = {va[i][0], va[i][1], va[i][2], va[i][3], vb[i][0], vb[i][1], vb[i][2], vb[i][3]};
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaxf(fmaf(v[e], sv[e], bv[e]), 0.f);
        {
          float vg[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) vg[e] = v[e];
          pt_range_guard<8>(vg, false, rng);
        }
        u32x4 hi, lo;
        pt_split8(v, hi, lo);
        const long pix = ((long)crop * Hq + (gy >> 1)) * Wq + (gx >> 1);
        u32x4* o = out + (pix * cout8 + (n0 >> 3) + eu) * 2;
        o[0] = hi;
        o[1] = lo;
      }
    }
  } else {
    // the chunk's staged rows of this thread, all requested before the first store
    constexpr int NIT = RCH / RSTEP;
    f32x4 va[NIT], vb[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) mm_lds_read32(mm_lds_addr(&Cs[(er0 + i * RSTEP) * CLD + eu * 8]), va[i], vb[i]);
    mm_lds_wait();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int rl = er0 + i * RSTEP;  // chunk-local
      const int r = ch * RCH + rl;
      int blk, y, x;
      pt_row_to_pixel<BS>(r >> 5, r & 31, blk, y, x);
      PT_BLK_PIXEL(blk, y, x)
      if (crop >= 0 && gy < H && gx < W) {
        f32x8 v = {va[i][0], va[i][1], va[i][2], va[i][3], vb[i][0], vb[i][1], vb[i][2], vb[i][3]};
        u32x4 hi, lo;
        if constexpr (RAW) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = fmaf(v[e], sv[e], bv[e]);
          hi = __builtin_bit_cast(u32x4, f32x4{v[0], v[1], v[2], v[3]});
          lo = __builtin_bit_cast(u32x4, f32x4{v[4], v[5], v[6], v[7]});
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = fmaxf(fmaf(v[e], sv[e], bv[e]), 0.f);
          {
            float vg[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) vg[e] = v[e];
            pt_range_guard<8>(vg, false, rng);
          }
          pt_split8(v, hi, lo);
        }
        const long pix = ((long)crop * H + gy) * W + gx;
        u32x4* o = out + (pix * cout8 + (n0 >> 3) + eu) * 2;
        // (regular stores: streaming stores, which the hq8 branch uses, measured +1.4 .. +4.6 % per layer at 4 pairs per
        // launch but -1.7 .. 0 % at the benchmark's 16 - profiles/HISTORY.md)
        o[0] = hi;
        o[1] = lo;
      }
    }
  }
  }  // chunks
  }
  PT_STAMP(4)
  mt = mt_next;
  nt = nt_next;
  wbase = wbase_next;
  if constexpr (OVL) {  // (X, Y, Z) <- (Z, X, Y)
    const int t = bufX;
    bufX = bufZ;
    bufZ = bufY;
    bufY = t;
  }
  if constexpr (!FUSE1) {
    if (chain) {  // the successor's slab 0 sits in pnext
      const int t = pcur;
      pcur = pnext;
      pnext = t;
    } else if (has_next) {  // (8x8-block variants only) another pixel tile: it starts with a load prologue
      wbase = wp + (long)(nt_next * BN) * (cin8 * 2);
      compute_poff(mt_next);
    }
  }
  // LDS-only: the staging area is the successor's next patch buffer (FUSE1: the next tile's raw window / patches);
  // the tile's own stores drain under the next tile, the raw-window registers are waited for where they are used
  mm_lds_barrier();
  PT_STAMP(5)
  PT_COUNT_ITEM()
