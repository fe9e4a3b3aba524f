// conv3x3_hl16_patch_kernel, part 3 of 6.  Fragment reads and matrix instructions of a half stage: a_addr / a_imm
// (LDS address of the tap-shifted activation fragment), read_one / read_frags (activation and weight fragments,
// double-buffered in registers), mma_one (the three f16 MFMAs of a product - or, hq8: two f16 + one block-scaled fp8).
  // ---------------- fragment read state --------------------------------------------------------------
  // A (patch) read of tap (ty, tx), k-step j, lane half h: pixel n = n0 + ty*PW + tx, piece
  // (4j + 2h) ^ swz(py + ty, px + tx).  swz(.., ty odd) = swz(.., ty even) ^ 4, so per row three lane
  // values a_sx[tx] = ((swz(py, px + tx) ^ 2h) << 4) cover every tap: byte offset inside the record =
  // a_sx[tx] ^ (64 * (j ^ (ty & 1))); the tap's pixel offset is an immediate.
  // WHOLE: no halo in LDS.  The swizzle depends on the row only: a_sx[tm][ty] = ((swz(blk, y + ty - 1) ^ 2h) << 4); the
  // tap's record is a_base + ((ty - 1) * BS + tx - 1) * 128 when the source pixel lies inside the block (bit `tap` of
  // a_ok) and otherwise the zero page, at the slot the pixel WOULD occupy (a_zb: its record parity for tx = 1, flipped
  // for tx = 0 / 2), so that the sixteen lanes of a read group stay on sixteen different slots.
  int a_base[TM], a_sx[TM][3];
  int a_ok[TM], a_zb[TM];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) {
    int blk, y, x;
    pt_row_to_pixel<BS>(wm * TM + tm, lr, blk, y, x);
    a_base[tm] = (blk * G::PP + y * G::PW + x) * P_ROWB;
    if constexpr (G::WHOLE) {
      a_ok[tm] = 0;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int sy = y + t / 3 - 1, sx = x + t % 3 - 1;
        if ((unsigned)sy < (unsigned)BS && (unsigned)sx < (unsigned)BS) a_ok[tm] |= 1 << t;
      }
      a_zb[tm] = ZOFF + ((x & 1) << 7);
#pragma unroll
      for (int ty = 0; ty < 3; ++ty) a_sx[tm][ty] = (pt_swz_w<BS>(blk, y + ty - 1) ^ (Q8 ? h : 2 * h)) << 4;
    } else {
      a_ok[tm] = 0;
      a_zb[tm] = 0;
#pragma unroll
      for (int tx = 0; tx < 3; ++tx) a_sx[tm][tx] = (pt_swz_a(y, x + tx) ^ (Q8 ? h : 2 * h)) << 4;  // Q8: fp16 piece 2j+h
    }
  }
  // record address (without the buffer-independent immediate of the haloed geometries) and swizzled piece offset of
  // k-step 0 of one activation fragment read
  auto a_addr = [&](auto TMC, auto TAPC, int pb, int& rec, int& sxo) {
    constexpr int tm = decltype(TMC)::value;
    constexpr int tap = decltype(TAPC)::value;
    constexpr int ty = tap / 3, tx = tap % 3;
    if constexpr (G::WHOLE) {
      constexpr int imm = ((ty - 1) * BS + (tx - 1)) * P_ROWB;
      const int inside = pb + a_base[tm] + imm;
      const int outside = (tx == 1) ? a_zb[tm] : (a_zb[tm] ^ 128);
      rec = ((a_ok[tm] >> tap) & 1) ? inside : outside;
      sxo = a_sx[tm][ty];
    } else {
      rec = pb + a_base[tm];
      sxo = a_sx[tm][tx] ^ (64 * (ty & 1));
    }
  };
  constexpr auto a_imm = [](int tap) constexpr -> int {  // folded into the ds_read offset field
    return G::WHOLE ? 0 : ((tap / 3) * G::PW + (tap % 3)) * P_ROWB;
  };
  int b_off[TN];  // weight row record + swizzled piece of k-step 0 (k-step 1: ^ 64)
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) {
    const int r = wn * TN * 32 + tn * 32 + lr;
    b_off[tn] = r * P_ROWB + ((((Q8 ? h : 2 * h)) ^ pt_swz_b(r)) << 4);
  }

  using I0 = std::integral_constant<int, 0>;
  struct Frags {
    f16x8 ah[TM], al[TM], bh[TN], bl[TN];  // Q8: ah/al = fp16 hi of k-step 0/1 (same for b); a8/b8 = fp8 operands
    i32x8 a8[TM], b8[TN];
  };
  constexpr int NPROD = TM * TN;          // products per 16-channel step: 4 / 2
  constexpr int NMMA = 3 * NPROD;         // MFMAs per half stage: 12 / 6
  constexpr int NMMA1 = Q8 ? 2 * NPROD : NMMA;  // Q8: first half = the fp16 hi*hi MFMAs of both k-steps
  constexpr int NMMA2 = Q8 ? NPROD : NMMA;      //     second half = one K=64 fp8 MFMA per product
  constexpr int NRD = 2 * TM + 2 * TN;    // ds_read_b128 per half stage: 8 / 6
  // one fragment read: r < 2*TM -> activation row block r/2 (hi, lo); else weight row block (hi, lo)
  auto read_one = [&](Frags& f, auto RC, auto TAPC, auto JC, int pb) {
    constexpr int r = decltype(RC)::value;
    constexpr int tap = decltype(TAPC)::value;
    constexpr int j = decltype(JC)::value;
    constexpr int ty = tap / 3, tx = tap % 3;
    if constexpr (Q8) {
      // JC = 0: fp16 fragments of both k-steps (piece 2*js + h); JC = 1: fp8 operands (pieces 4 + 2h + q)
      constexpr int sel = r % 2;  // k-step (fp16) or 16-byte half q of the 32-byte fp8 fragment
      if constexpr (r < 2 * TM) {
        constexpr int tm = r / 2;
        int rec, sxo;
        a_addr(std::integral_constant<int, tm>{}, TAPC, pb, rec, sxo);
        rec += a_imm(tap);
        if constexpr (j == 0) {
          const f16x8 v = *reinterpret_cast<const f16x8*>(smem + rec + (sxo ^ (32 * sel)));
          if constexpr (sel == 0) f.ah[tm] = v; else f.al[tm] = v;
        } else {
          const u32x4 v = *reinterpret_cast<const u32x4*>(smem + rec + (sxo ^ 64 ^ ((h ^ (2 * h)) << 4) ^ (16 * sel)));
#pragma unroll
          for (int e = 0; e < 4; ++e) f.a8[tm][4 * sel + e] = (int)v[e];
        }
      } else {
        constexpr int tn = (r - 2 * TM) / 2;
        constexpr int sb = RING0 + (tap % 3) * B_BYTES;
        if constexpr (j == 0) {
          const f16x8 v = *reinterpret_cast<const f16x8*>(smem + (b_off[tn] ^ (32 * sel)) + sb);
          if constexpr (sel == 0) f.bh[tn] = v; else f.bl[tn] = v;
        } else {
          const u32x4 v = *reinterpret_cast<const u32x4*>(smem + (b_off[tn] ^ 64 ^ ((h ^ (2 * h)) << 4) ^ (16 * sel)) + sb);
#pragma unroll
          for (int e = 0; e < 4; ++e) f.b8[tn][4 * sel + e] = (int)v[e];
        }
      }
    } else if constexpr (r < 2 * TM) {
      constexpr int tm = r / 2;
      // record offsets are multiples of 128 and the swizzled piece offset is < 128: xor 16 flips hi <-> lo
      int rec, sxo;
      a_addr(std::integral_constant<int, tm>{}, TAPC, pb, rec, sxo);
      sxo ^= 64 * j;
      constexpr int imm = a_imm(tap);
      if constexpr (r % 2 == 0) f.ah[tm] = *reinterpret_cast<const f16x8*>(smem + (rec + sxo) + imm);
      else f.al[tm] = *reinterpret_cast<const f16x8*>(smem + (rec + (sxo ^ 16)) + imm);
    } else {
      constexpr int tn = (r - 2 * TM) / 2;
      constexpr int sb = RING0 + (tap % 3) * B_BYTES;
      const int xo = b_off[tn] ^ (64 * j);
      if constexpr (r % 2 == 0) f.bh[tn] = *reinterpret_cast<const f16x8*>(smem + xo + sb);
      else f.bl[tn] = *reinterpret_cast<const f16x8*>(smem + (xo ^ 16) + sb);
    }
  };
  // one MFMA of a half stage, term-major so that consecutive MFMAs hit different accumulators:
  // i -> term i / NPROD (lo*hi, hi*lo, hi*hi), product i % NPROD
  auto mma_one = [&](const Frags& f, auto IC, auto HALFC) {
    constexpr int i = decltype(IC)::value;
    constexpr int half = decltype(HALFC)::value;
    constexpr int term = i / NPROD, p = i % NPROD;
    constexpr int tm = p / TN, tn = p % TN;
    if constexpr (Q8) {
      if constexpr (half == 0) {  // fp16 hi*hi, k-step = term (0 / 1)
        if constexpr (term == 0)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[tm], f.bh[tn], acc[tm][tn], 0, 0, 0);
        else
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.al[tm], f.bl[tn], acc[tm][tn], 0, 0, 0);
      } else {                    // fp8 correction: K = 64 = [a8 . w_lo8 | a_lo8 . w8], block scale 2^-3
        acc[tm][tn] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(f.a8[tm], f.b8[tn], acc[tm][tn], 0, 0, 0,
                                                                      Q8_SCALE_A, 0, Q8_SCALE_B);
      }
    } else if constexpr (term == 0)
      acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.al[tm], f.bh[tn], acc[tm][tn], 0, 0, 0);
    else if constexpr (term == 1)
      acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[tm], f.bl[tn], acc[tm][tn], 0, 0, 0);
    else
      acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[tm], f.bh[tn], acc[tm][tn], 0, 0, 0);
  };
  // ---------------- M16: the same fragments as operands of v_mfma_f32_16x16x32_f16 -------------------------
  // A 32x32x16 fragment is 4 VGPRs: lane l = row l % 32, the 8 channels of lane half l / 32 of its k-step.  In 16-lane
  // rows the pair (k-step 0, k-step 1) of one 32-row block is
  //     R0 = [rows 0-15, (j0,h0) | rows 16-31, (j0,h0) | rows 0-15, (j0,h1) | rows 16-31, (j0,h1)]      R1 = the same for j1.
  // v_permlane16_swap_b32 exchanges the odd 16-lane rows of its first register with the even ones of its second:
  //     R0 = [rows 0-15: (j0,h0) | (j1,h0) | (j0,h1) | (j1,h1)]                                         R1 = the same for rows 16-31
  // - each a 16x16x32 operand (lane l = row l % 16, k-group l / 16) whose four k-groups cover the 32 channels of the slab.
  // Activations and weights are paired the same way, so both operands agree on the order of the k-groups (which a dot
  // product does not care about).  Reads, addresses and swizzles are those of read_one; four swaps per pair follow.
  // An operand = the hi and lo fragments of both k-steps of ONE 32-row block (16 VGPRs): x[j] as read, x[si] (16-row
  // half) once swapped.
  struct Opnd {
    u32x4 h[2], l[2];
  };
  // read k of an operand: 0 = hi j0, 1 = hi j1, 2 = lo j0, 3 = lo j1 (a swap pair completes with every second read)
  auto m16_read = [&](Opnd& o, auto ISAC, auto TILEC, auto KC, auto TAPC, int pb) {
    constexpr bool isa = decltype(ISAC)::value != 0;
    constexpr int tile = decltype(TILEC)::value;
    constexpr int k = decltype(KC)::value;
    constexpr int tap = decltype(TAPC)::value;
    constexpr int j = k & 1, lo = k >> 1;
    int ad;
    if constexpr (isa) {
      int rec, sxo;
      a_addr(std::integral_constant<int, tile>{}, TAPC, pb, rec, sxo);
      sxo ^= 64 * j;
      ad = (rec + (sxo ^ (16 * lo))) + a_imm(tap);
    } else {
      constexpr int sb = RING0 + (tap % 3) * B_BYTES;
      ad = ((b_off[tile] ^ (64 * j)) ^ (16 * lo)) + sb;
    }
    const u32x4 v = *reinterpret_cast<const u32x4*>(smem + ad);
    if constexpr (lo == 0) o.h[j] = v; else o.l[j] = v;
  };
  // swap k of an operand: register k & 3 of the hi (k < 4) or lo pair
  auto m16_swap = [&](Opnd& o, auto KC) {
    constexpr int k = decltype(KC)::value;
    constexpr int w = k & 3;
    if constexpr (k < 4) {
      const auto s = __builtin_amdgcn_permlane16_swap(o.h[0][w], o.h[1][w], false, false);
      o.h[0][w] = s[0];
      o.h[1][w] = s[1];
    } else {
      const auto s = __builtin_amdgcn_permlane16_swap(o.l[0][w], o.l[1][w], false, false);
      o.l[0][w] = s[0];
      o.l[1][w] = s[1];
    }
  };
  // MFMA i (0..11) of the product (tm, tn): term-major like mma_one (lo*hi, hi*lo, hi*hi), sub-tile i % 4 = 2 si + sj
  auto m16_mma = [&](const Opnd& a, const Opnd& b, auto TMC, auto TNC, auto IC) {
    constexpr int tm = decltype(TMC)::value, tn = decltype(TNC)::value;
    constexpr int i = decltype(IC)::value;
    constexpr int term = i / 4, si = (i >> 1) & 1, sj = i & 1;
    const f16x8 ah = __builtin_bit_cast(f16x8, a.h[si]), al = __builtin_bit_cast(f16x8, a.l[si]);
    const f16x8 bh = __builtin_bit_cast(f16x8, b.h[sj]), bl = __builtin_bit_cast(f16x8, b.l[sj]);
    f32x4& c = acc16[tm][tn][si][sj];
    if constexpr (term == 0) c = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, c, 0, 0, 0);
    else if constexpr (term == 1) c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, c, 0, 0, 0);
    else c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, c, 0, 0, 0);
  };
  // slot i of a half stage's load schedule for one operand: its four reads from slot R0 on (one per slot), its eight
  // swaps from slot S0 on (SPS per slot); each non-MFMA instruction pinned behind an MFMA like everything in the K loop
  auto m16_load_slot = [&](Opnd& o, auto ISAC, auto TILEC, auto TAPC, int pb, auto IC, auto R0C, auto S0C, auto SPSC) {
    constexpr int i = decltype(IC)::value, r0 = decltype(R0C)::value, s0 = decltype(S0C)::value;
    constexpr int sps = decltype(SPSC)::value;
    if constexpr (i >= r0 && i < r0 + 4) {
      m16_read(o, ISAC, TILEC, std::integral_constant<int, (i - r0) & 3>{}, TAPC, pb);
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (i >= s0 && i < s0 + 8 / sps) {
      constexpr int k0 = ((i - s0) * sps) & 7;
      m16_swap(o, std::integral_constant<int, k0>{});
      if constexpr (sps > 1) m16_swap(o, std::integral_constant<int, (k0 + 1) & 7>{});
      if constexpr (sps > 2) {
        m16_swap(o, std::integral_constant<int, (k0 + 2) & 7>{});
        m16_swap(o, std::integral_constant<int, (k0 + 3) & 7>{});
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // all of an operand at once (prologue)
  auto m16_load = [&](Opnd& o, auto ISAC, auto TILEC, auto TAPC, int pb) {
    m16_read(o, ISAC, TILEC, std::integral_constant<int, 0>{}, TAPC, pb);
    m16_read(o, ISAC, TILEC, std::integral_constant<int, 1>{}, TAPC, pb);
    m16_read(o, ISAC, TILEC, std::integral_constant<int, 2>{}, TAPC, pb);
    m16_read(o, ISAC, TILEC, std::integral_constant<int, 3>{}, TAPC, pb);
    m16_swap(o, std::integral_constant<int, 0>{});
    m16_swap(o, std::integral_constant<int, 1>{});
    m16_swap(o, std::integral_constant<int, 2>{});
    m16_swap(o, std::integral_constant<int, 3>{});
    m16_swap(o, std::integral_constant<int, 4>{});
    m16_swap(o, std::integral_constant<int, 5>{});
    m16_swap(o, std::integral_constant<int, 6>{});
    m16_swap(o, std::integral_constant<int, 7>{});
  };
  auto read_frags = [&](Frags& f, auto TAPC, auto JC, int pb) {  // all reads of a half stage (prologue)
    read_one(f, std::integral_constant<int, 0>{}, TAPC, JC, pb);
    read_one(f, std::integral_constant<int, 1>{}, TAPC, JC, pb);
    read_one(f, std::integral_constant<int, 2>{}, TAPC, JC, pb);
    read_one(f, std::integral_constant<int, 3>{}, TAPC, JC, pb);
    read_one(f, std::integral_constant<int, 4>{}, TAPC, JC, pb);
    read_one(f, std::integral_constant<int, 5>{}, TAPC, JC, pb);
    if constexpr (NRD > 6) {
      read_one(f, std::integral_constant<int, 6>{}, TAPC, JC, pb);
      read_one(f, std::integral_constant<int, 7>{}, TAPC, JC, pb);
    }
  };
