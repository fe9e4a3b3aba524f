// conv3x3_hl16_patch_kernel, part 4 of 6.  Prologue of a tile: successor lookup; first-tile loads; the fused first
// layer's conv1_1 (raw window -> 18 x 18 x 64 patch on the matrix cores, written into the LDS patch buffers: gather1 /
// mma1 / emit1) and pro_slot, the same computation for the SUCCESSOR tile cut into MFMA-slot-sized slices that ride in
// the K loop of the current tile (OVL).
  // ---------------- prologue: patch(slab 0), weight stages 0..2 --------------------------------------
  static_assert(G::BYTES % 256 == 0 && RING0 % 256 == 0 && B_BYTES % 256 == 0, "hi/lo xor addressing");
  const int nitem_ = item + (gridDim.x >> 3);
  const bool has_next = nitem_ < clen;
  int mt_next = 0, nt_next = 0;
  if (has_next) decode_item(nitem_, mt_next, nt_next);
  if constexpr (STREAM) {
    if (has_next) {
      TileBlocks tb;
      tile_blocks(mt_next, tb);
      unsigned* pk = reinterpret_cast<unsigned*>(smem + POFF_OFF) + tid;
      pk[0 * 512] = poff_round(std::integral_constant<int, 0>{}, tb);
      pk[1 * 512] = poff_round(std::integral_constant<int, 1>{}, tb);
      pk[2 * 512] = poff_round(std::integral_constant<int, 2>{}, tb);
      pk[3 * 512] = poff_round(std::integral_constant<int, 3>{}, tb);
      if constexpr (G::PA > 4) pk[4 * 512] = poff_round(std::integral_constant<int, 4>{}, tb);
      if constexpr (G::PA > 5) pk[5 * 512] = poff_round(std::integral_constant<int, 5>{}, tb);
      if constexpr (G::PA > 6) pk[6 * 512] = poff_round(std::integral_constant<int, 6>{}, tb);
    }
  }
  float c11max = 0.f;  // range guard of the conv1_1 outputs (pt_range[2])
  // OVL: the successor's block origin (its conv1_1 patches are made under this tile's K loop) and the tile after it
  // (whose raw window is fetched meanwhile)
  int nx_gy0 = 0, nx_gx0 = 0;
  bool nx_valid = false, has_next2 = false;
  int mt_next2 = 0;
  if constexpr (OVL) {
    if (has_next) {
      const int crop = mt_next / nbpc, br = mt_next - crop * nbpc;
      const int by = br / nbx;
      nx_gy0 = by * 16 - 1;
      nx_gx0 = (br - by * nbx) * 16 - 1;
      nx_valid = mt_next < nblk;
      const int nitem2_ = nitem_ + (gridDim.x >> 3);
      has_next2 = nitem2_ < clen;
      int nt2_ = 0;
      if (has_next2) decode_item(nitem2_, mt_next2, nt2_);
    }
    pcur = bufX;
    pnext = bufY;
  }
  if constexpr (FUSE1) {
  if (!OVL || !primed) {  // OVL: only the first tile of a workgroup computes its own patches up front
    if constexpr (!OVL) {
      pcur = P0_OFF;
      pnext = P1_OFF;
    }
    // ---- raw window: image rows by*16-2 .. +19, columns bx*16-2 .. +19 of the 3 colour planes (zero outside) ----
    float* R = reinterpret_cast<float*>(smem + RAW_OFF);
    const int b0 = mt;  // NB == 1
    const int crop0 = b0 / nbpc, br0 = b0 - crop0 * nbpc;
    const int by0 = br0 / nbx, bx0 = br0 - by0 * nbx;
    if (!raw_ready) fetch_raw(b0);  // first tile of this workgroup
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (tid + 512 * k < 1200) R[tid + 512 * k] = raw_value(b0, k);
    if constexpr (OVL) {
      if (has_next) fetch_raw(mt_next);  // older than the ring loads below: landed when the counted wait passes
    }
    issue_b(0, 0, 0);  // conv1_2's weight ring flies while the patch is computed
    issue_b(1, 0, 1);
    issue_b(2, 0, 2);
    __syncthreads();
    if constexpr (OVL) {  // the overlapped rounds take their weight fragments from registers
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) {
        w1h[mb] = *reinterpret_cast<const f16x8*>(smem + W1_OFF + ((mb * 64 + lane) * 2) * 16);
        w1l[mb] = *reinterpret_cast<const f16x8*>(smem + W1_OFF + ((mb * 64 + lane) * 2 + 1) * 16);
      }
    }
    // ---- conv1_1 on the 324 patch pixels as C^T = W1 X^T: MFMA rows = channels, columns = pixels, so a lane
    // ends up with ONE pixel (lane & 15 of pixel tile g) and, per 16-channel block, 4 consecutive channels: their
    // hi and lo halves leave as two 8-byte LDS stores and all per-pixel work (coordinates, swizzle, image
    // mask) is done once per lane.  16-pixel tiles (16x16x32 MFMA, K = 32 in one step): 21 tiles over 8 waves =
    // at most 3 per wave (32-pixel tiles: 11 tiles, two waves' worth of work for waves 0-2 while 3-7 wait). ----
    const int l15 = lane & 15, kg1 = lane >> 4;
    // Three rounds per wave (tiles wave, wave + 8, wave + 16; waves 5-7 have two), written branch-free so that the
    // scheduler overlaps the LDS gather of round i + 1 with the matrix-core chain and the VALU epilogue of round i
    // (two waves per SIMD hide nothing of a dependent ds_read -> cvt -> MFMA x3 -> VALU chain on their own):
    //  * the folded bias is the INITIAL VALUE of the accumulators (binit, 16 registers for the whole kernel) - no LDS
    //    read and no fma in the epilogue, the 2^-shift of the weights is one packed multiply;
    //  * patch pixels outside the image (conv1_2's zero padding applies to conv1_1's OUTPUT) get 0 as the upper bound of
    //    the ReLU / fp16-range clamp - the mask costs no instruction;
    //  * lanes past pixel 323 (last tile) recompute pixel 323 and store the same bytes to the same place.
    auto gather1 = [&](int g, f16x8& xh, f16x8& xl) {
      const int n = g * 16 + l15;
      const int nc = n < 324 ? n : 323;
      const int ppy = nc / 18, ppx = nc - ppy * 18;
      const int rbase = ppy * 20 + ppx;  // window position of tap (0,0)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = R[rbase + roff[e]];
        if (e == 3 && kg1 == 3) v = 1.f;  // k = 27: the bias slot
        xh[e] = (_Float16)v;
        xl[e] = mm_hl_lo(v, xh[e]);
      }
    };
    auto mma1 = [&](const f16x8& xh, const f16x8& xl, f32x4 (&c1)[4]) {
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) {
        const f16x8 w1h = *reinterpret_cast<const f16x8*>(smem + W1_OFF + ((mb * 64 + lane) * 2) * 16);
        const f16x8 w1l = *reinterpret_cast<const f16x8*>(smem + W1_OFF + ((mb * 64 + lane) * 2 + 1) * 16);
        c1[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1l, xh, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        c1[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1h, xl, c1[mb], 0, 0, 0);
        c1[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1h, xh, c1[mb], 0, 0, 0);
      }
    };
    auto emit1 = [&](int g, const f32x4 (&c1)[4]) {
      const int n0_ = g * 16 + l15;
      const int n = n0_ < 324 ? n0_ : 323;
      const int ppy = n / 18, ppx = n - ppy * 18;
      const int gy = by0 * 16 - 1 + ppy, gx = bx0 * 16 - 1 + ppx;
      const bool inimg = (b0 < nblk) && ((unsigned)gy < (unsigned)H) && ((unsigned)gx < (unsigned)W);
      const float top = inimg ? 65504.f : 0.f;  // fp16 maximum (the guard below reports anything above PT_SAT_FP16)
      const int sw = pt_swz_a(ppy, ppx);
      const int hh = kg1 & 1;  // which half (4 channels) of an 8-channel unit
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) {  // channels 16 mb + 4 kg1 .. + 3 = slab mb >> 1, unit q, half hh
        const int q = (mb & 1) * 2 + (kg1 >> 1);
        const int rb = ((mb >> 1) == 0 ? pcur : pnext) + n * P_ROWB;  // this pixel's record in slab mb >> 1
        f16x4 hi, lo;
        float vv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = c1[mb][r] * fz.oscale1;
          v = __builtin_amdgcn_fmed3f(v, 0.f, top);  // ReLU, the fp16 range clamp and the image mask in one instruction
          c11max = fmaxf(c11max, v);
          vv[r] = v;
          hi[r] = (_Float16)v;
          lo[r] = mm_hl_lo(v, hi[r]);
        }
        if constexpr (Q8) {
          // record = [fp16 hi: pieces 0..3 | e4m3(a/4): pieces 4,5 | e4m3(a_lo*512): pieces 6,7]
          *reinterpret_cast<f16x4*>(smem + rb + ((q ^ sw) << 4) + 8 * hh) = hi;
          int pa = 0, pl = 0;
          pa = __builtin_amdgcn_cvt_pk_fp8_f32(fminf(vv[0] * 0.25f, 448.f), fminf(vv[1] * 0.25f, 448.f), pa, false);
          pa = __builtin_amdgcn_cvt_pk_fp8_f32(fminf(vv[2] * 0.25f, 448.f), fminf(vv[3] * 0.25f, 448.f), pa, true);
          float ll[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) ll[r] = __builtin_amdgcn_fmed3f((vv[r] - (float)hi[r]) * 512.f, -448.f, 448.f);
          pl = __builtin_amdgcn_cvt_pk_fp8_f32(ll[0], ll[1], pl, false);
          pl = __builtin_amdgcn_cvt_pk_fp8_f32(ll[2], ll[3], pl, true);
          const int bo = 8 * (q & 1) + 4 * hh;  // byte of channel 8q + 4hh inside its 16-channel piece
          *reinterpret_cast<int*>(smem + rb + (((4 + (q >> 1)) ^ sw) << 4) + bo) = pa;
          *reinterpret_cast<int*>(smem + rb + (((6 + (q >> 1)) ^ sw) << 4) + bo) = pl;
        } else {
          *reinterpret_cast<f16x4*>(smem + rb + hh * 8 + (((2 * q) ^ sw) << 4)) = hi;
          *reinterpret_cast<f16x4*>(smem + rb + hh * 8 + (((2 * q + 1) ^ sw) << 4)) = lo;
        }
      }
    };
    if constexpr (OVL) {  // once per workgroup: plain rounds (the register budget belongs to the overlapped form)
#pragma nounroll
      for (int g = wave; g < 21; g += 8) {
        f16x8 xh0, xl0;
        f32x4 ca[4];
        gather1(g, xh0, xl0);
        mma1(xh0, xl0, ca);
        emit1(g, ca);
      }
    } else {
      f16x8 xh0, xl0, xh1, xl1;
      f32x4 ca[4], cb[4];
      gather1(wave, xh0, xl0);
      gather1(wave + 8, xh1, xl1);
      mma1(xh0, xl0, ca);
      mma1(xh1, xl1, cb);
      const bool third = wave + 16 < 21;  // wave-uniform
      if (third) gather1(wave + 16, xh0, xl0);
      emit1(wave, ca);
      if (third) mma1(xh0, xl0, ca);
      emit1(wave + 8, cb);
      if (third) emit1(wave + 16, ca);
    }
    if (c11max > (Q8 ? PT_SAT_E4M3 : PT_SAT_FP16)) atomicAdd(&rng[2], 1u);
    c11max = 0.f;
    mm_wait_vm<2 * NBL>();  // weight stage 0 landed (this wave's part)
    __syncthreads();        // both patch slabs are complete
    if constexpr (OVL) {
      if (has_next) {  // the successor's raw window (every wave is past its gathers from the old one)
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (tid + 512 * k < 1200) R[tid + 512 * k] = raw_value(mt_next, k);
      }
    }
  }
  PT_STAMP(1)
  } else {
    if (!primed) {  // first tile of this workgroup
      issue_tile_head(pcur);
      PT_STAMP(0)
      mm_wait_vm<2 * NBL>();  // patch + weight stage 0 landed (this wave's part)
      __builtin_amdgcn_s_barrier();
    }
    PT_STAMP(1)
  }
  Frags f0, f1;
  // M16: the operands of a stage (see the K loop): oA[tm] (BN = 128) or the two alternating sets of the single
  // activation block (BN = 64), oB[tn]; every tile starts with the first stage's first product, (oA[0], oB[0])
  Opnd oA[2], oB[2];
  if constexpr (M16) {
    m16_load(oA[0], std::integral_constant<int, 1>{}, I0{}, I0{}, pcur);
    m16_load(oB[0], I0{}, I0{}, I0{}, pcur);
  } else {
    read_frags(f0, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, pcur);
  }

  // One stage = one (slab, tap): 2 k-steps of 16 channels.  Weight stage t+3 is issued after the
  // barrier of stage t (its ring slot was last read by stage t); the patch of the next slab is issued
  // round by round in taps 0..PA-1, BEFORE the weights of the same stage so that the counted vmcnt of
  // a later barrier retires it as well.
  // MODE 0: a slab with something to prefetch - patch slab `pslab` (of the tile poff describes) and, once the
  // weight stream passes tap 8, weights (wb2, slab ws2).  Interior slab: pslab = ws2 = slab + 1, wb2 = wbase.
  // Transition slab (last slab of a tile that has a successor): poff = the successor's table, pslab = ws2 = 0,
  // wb2 = the successor's weights - the same code, so every counted vmcnt is the interior one.
  // MODE 1: last slab of the workgroup's last tile (nothing to prefetch).
  // OVL: one 16-pixel conv1_1 round of the SUCCESSOR tile (see the serial form above) cut into 36 slices = the MFMA
  // slots of three stages; round rr of a wave runs in stages 3 rr .. 3 rr + 2 of the current tile's second slab.
  //   0: pixel of this lane            1-4: window gather (2 values each)     5: image mask, swizzle
  //   6-9: hi/lo split of the gathered values (2 each)                        12-23: the 12 MFMAs (16x16x32)
  //   15-30: one output value per slot (scale, ReLU/clamp/mask, hi/lo split), 8-byte stores after each fourth
  // Slab 0 of the successor (channels 0-31) goes to bufZ, slab 1 to bufX (this tile's first slab: dead).
  int pr_ppy = 0, pr_ppx = 0, pr_rbase = 0, pr_rec = 0, pr_sw = 0;
  float pr_top = 0.f;
  float pr_v[8];
  f16x8 pr_xh, pr_xl;
  f32x4 pr_c[4];
  f16x4 pr_hi, pr_lo;
  auto pro_slot = [&](auto SC, auto RC) {
    constexpr int sl = decltype(SC)::value;
    constexpr int rr = decltype(RC)::value;
    if constexpr (OVL) {
      const float* R = reinterpret_cast<const float*>(smem + RAW_OFF);
      if constexpr (sl == 0) {
        const int g0 = wave + 8 * rr;
        const int g = g0 < 21 ? g0 : 20;  // waves 5-7 repeat tile 20 in their third round (same bytes, same place)
        // laundered lane id: everything below depends on the lane only, would be hoisted out of the tile loop for all
        // three rounds and spilled (scratch reloads with vmcnt(0) inside the K loop)
        int lane_ = lane;
        asm volatile("" : "+v"(lane_));
        const int n = g * 16 + (lane_ & 15);
        const int nc = n < 324 ? n : 323;
        pr_ppy = nc / 18;
        pr_ppx = nc - pr_ppy * 18;
        pr_rbase = pr_ppy * 20 + pr_ppx;
        pr_rec = nc * P_ROWB;
      } else if constexpr (sl >= 1 && sl <= 4) {
        constexpr int e = 2 * (sl - 1);
        pr_v[e] = R[pr_rbase + roff[e]];
        pr_v[e + 1] = R[pr_rbase + roff[e + 1]];
        if constexpr (e + 1 == 3) {
          if ((lane >> 4) == 3) pr_v[3] = 1.f;  // k = 27: the bias slot
        }
      } else if constexpr (sl == 5) {
        const int gy = nx_gy0 + pr_ppy, gx = nx_gx0 + pr_ppx;
        const bool inimg = nx_valid & ((unsigned)gy < (unsigned)H) & ((unsigned)gx < (unsigned)W);  // no branches
        pr_top = inimg ? 65504.f : 0.f;
        pr_sw = pt_swz_a(pr_ppy, pr_ppx);
      } else if constexpr (sl >= 6 && sl <= 9) {
        constexpr int e = 2 * (sl - 6);
#pragma unroll
        for (int k = e; k < e + 2; ++k) {
          pr_xh[k] = (_Float16)pr_v[k];
          pr_xl[k] = (_Float16)(pr_v[k] - (float)pr_xh[k]);
        }
      }
      if constexpr (sl >= 12 && sl <= 23) {
        constexpr int mb = (sl - 12) / 3, term = (sl - 12) % 3;
        if constexpr (term == 0)
          pr_c[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1l[mb], pr_xh, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        else if constexpr (term == 1)
          pr_c[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1h[mb], pr_xl, pr_c[mb], 0, 0, 0);
        else
          pr_c[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1h[mb], pr_xh, pr_c[mb], 0, 0, 0);
      }
      if constexpr (sl >= 15 && sl <= 30) {
        constexpr int mb = (sl - 15) / 4, r = (sl - 15) % 4;
        float v = pr_c[mb][r] * fz.oscale1;
        v = __builtin_amdgcn_fmed3f(v, 0.f, pr_top);
        c11max = fmaxf(c11max, v);
        pr_hi[r] = (_Float16)v;
        pr_lo[r] = mm_hl_lo(v, pr_hi[r]);
        if constexpr (r == 3) {
          const int kg1 = lane >> 4;
          const int q = (mb & 1) * 2 + (kg1 >> 1);
          const int rb = ((mb >> 1) == 0 ? bufZ : bufX) + pr_rec + (kg1 & 1) * 8;
          *reinterpret_cast<f16x4*>(smem + rb + (((2 * q) ^ pr_sw) << 4)) = pr_hi;
          *reinterpret_cast<f16x4*>(smem + rb + (((2 * q + 1) ^ pr_sw) << 4)) = pr_lo;
        }
      }
    }
  };
