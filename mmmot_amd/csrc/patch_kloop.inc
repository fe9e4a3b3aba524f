// conv3x3_hl16_patch_kernel, part 5 of 6.  The K loop: stage (one (tap, slab) step: 2 x 16 channels, one s_barrier,
// counted vmcnt, loads of stage t + 3 and the next patch round issued between the MFMAs), slab_body (nine taps), the
// slab loop with the transition slab that streams the successor tile's first stage in (chained tiles).
  bool rawfly = false;  // OVL: three raw-window loads were issued in stage 0 of the second slab (counted waits below)
  auto stage = [&](auto TAPC, auto MODEC, auto PROC, auto SPARC, int slab, int pslab, const u32x4* wb2, int ws2) {
    constexpr int tap = decltype(TAPC)::value;
    constexpr int PAR = (tap + decltype(SPARC)::value) & 1;  // M16: stage parity = (9 slab + tap) & 1 (SPARC = slab & 1)
    constexpr int NSL16 = 12 * TM;                           // M16: MFMA slots per half stage (24 / 12)
    constexpr int MODE = decltype(MODEC)::value;
    constexpr bool PRO = decltype(PROC)::value != 0;  // OVL: the successor's conv1_1 slices ride in the MFMA slots
    constexpr bool last = (MODE == 1);
    // loads this wave issued one stage earlier (they may stay in flight across this stage's barrier)
    constexpr int ptap = (tap + 8) % 9;  // tap of the previous stage
    constexpr int prev_issued =
        (tap == 0) ? NBL  // previous stage = tap 8 of a non-last slab (or the prologue's stage-2 weights)
                   : (((last || FUSE1) ? 0 : (ptap < G::PA ? 1 : 0)) + ((last && ptap + 3 > 8) ? 0 : NBL));
    // Half stages are written as ONE MFMA + ONE other instruction at a time (sched_barrier pins the order):
    // the two waves of a SIMD run in lockstep after every barrier, so any run of non-MFMA issue (8 ds_reads,
    // an LDS-DMA with its address math) leaves the matrix pipe idle unless it is cut into MFMA-sized gaps.
    // first half: MFMAs of the first 16-channel step, fragments of the second step read underneath
    auto half1 = [&](auto IC) {
      constexpr int i = decltype(IC)::value;
      if constexpr (i < NMMA1) {
        mma_one(f0, IC, I0{});
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (i < NRD) {
        read_one(f1, IC, TAPC, std::integral_constant<int, 1>{}, pcur);
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (PRO && i < 6) {
        pro_slot(std::integral_constant<int, (tap % 3) * 12 + i>{}, std::integral_constant<int, tap / 3>{});
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    // M16 (16x16x32 MFMAs need both k-steps of their operands, so "compute k-step 0 while k-step 1 loads" becomes
    // "compute one product while the operands of the next are loaded and swapped"): a stage is cut into its products -
    // 12 MFMAs each - in an order in which consecutive products share an operand, and an operand's registers are
    // reloaded one to two products after their last use, so the 64 fragment registers do not grow.  BN = 128, parity p:
    //     (0, p) (0, 1-p) | barrier | (1, 1-p) (1, p)        loads: oB[1-p], oA[1] (this stage's) | oA[0], oB[1-p] (next stage's)
    // - the next stage starts with (0, 1-p), the two operands the last product does NOT use, hence the parity: it
    // alternates from stage to stage and is 0 at every tile's first stage (an even number of stages per tile:
    // mmmot_patch_m16).  BN = 64 has one activation block: (0, 0) | barrier | (0, 1) on the activation set oA[p], the
    // other set and oB[0] reloaded in the second half, oB[1] in the first.
    // As in the 32x32x16 form every read of stage t + 1 follows barrier t and has landed before barrier t + 1.
    auto m16_half1 = [&](auto IC) {
      constexpr int i = decltype(IC)::value;
      using I1 = std::integral_constant<int, 1>;
      if constexpr (TM == 2) {
        using PN = std::integral_constant<int, 1 - PAR>;
        if constexpr (i < 12) m16_mma(oA[0], oB[PAR], I0{}, std::integral_constant<int, PAR>{}, IC);
        else m16_mma(oA[0], oB[1 - PAR], I0{}, PN{}, std::integral_constant<int, (i - 12) % 12>{});
        __builtin_amdgcn_sched_barrier(0);
        m16_load_slot(oB[1 - PAR], I0{}, PN{}, TAPC, pcur, IC, I0{}, std::integral_constant<int, 8>{},
                      std::integral_constant<int, 2>{});
        m16_load_slot(oA[1], I1{}, I1{}, TAPC, pcur, IC, std::integral_constant<int, 12>{},
                      std::integral_constant<int, 20>{}, std::integral_constant<int, 2>{});
      } else {
        m16_mma(oA[PAR], oB[0], I0{}, I0{}, IC);
        __builtin_amdgcn_sched_barrier(0);
        m16_load_slot(oB[1], I0{}, I1{}, TAPC, pcur, IC, I0{}, std::integral_constant<int, 8>{},
                      std::integral_constant<int, 2>{});
      }
    };
    if constexpr (M16) {
      pt_unroll(std::make_integer_sequence<int, NSL16>{}, m16_half1);
    } else {
    half1(std::integral_constant<int, 0>{});
    half1(std::integral_constant<int, 1>{});
    half1(std::integral_constant<int, 2>{});
    half1(std::integral_constant<int, 3>{});
    half1(std::integral_constant<int, 4>{});
    half1(std::integral_constant<int, 5>{});
    half1(std::integral_constant<int, 6>{});
    half1(std::integral_constant<int, 7>{});
    half1(std::integral_constant<int, 8>{});
    half1(std::integral_constant<int, 9>{});
    half1(std::integral_constant<int, 10>{});
    half1(std::integral_constant<int, 11>{});
    }
    if constexpr (PRO && (tap == 1 || tap == 2)) {
      // the three raw-window loads of stage 0 are younger than the weights this barrier needs: they may stay in flight
      if (rawfly) mm_wait_vm<prev_issued + 3>();
      else mm_wait_vm<prev_issued>();
    } else mm_wait_vm<prev_issued>();  // weights of stage t+1 (and every older load) landed
    // lgkmcnt(0) as a compiler-visible s_waitcnt (vmcnt 63 / expcnt 7 / lgkmcnt 0): the waitcnt pass then
    // knows the second step's fragments have landed and does not re-wait after the next reads are issued
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();
    // second half: MFMAs of the second step; first step of the next stage read underneath; this stage's
    // loads (patch round first, then the weights of stage t+3) issued at three spread-out points
    auto issue_at = [&](auto IC, auto ATPC, auto ATB0C, auto ATB1C) {  // the DMA issue points among the slots of the half
      constexpr int i = decltype(IC)::value;
      constexpr int at_patch = decltype(ATPC)::value, at_b0 = decltype(ATB0C)::value, at_b1 = decltype(ATB1C)::value;
      if constexpr (i == at_patch) {
        if constexpr (!FUSE1 && !last && tap < G::PA) issue_patch_round(TAPC, pslab, pnext);
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (i == at_b0 || (i == at_b1 && NBL > 1)) {
        using BI = std::integral_constant<int, (i == at_b0) ? 0 : 1>;
        if constexpr (tap + 3 <= 8) issue_b1(BI{}, wbase, tap + 3, slab, tap % 3);
        else if constexpr (MODE == 0) issue_b1(BI{}, wb2, tap + 3 - 9, ws2, tap % 3);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    // M16 second half.  BN = 128: products (1, 1 - p), (1, p); oA[0] and then oB[1 - p] (free after the first of the two
    // products) take the NEXT stage's fragments - its first product is (0, 1 - p).  BN = 64: product (0, 1); the other
    // activation set and oB[0] take the next stage's.  The DMA issue points sit at twice their 32x32x16 slot numbers
    // (an MFMA is half as long), moved off the slots that carry a read or a swap.
    auto m16_half2 = [&](auto IC) {
      constexpr int i = decltype(IC)::value;
      using I1 = std::integral_constant<int, 1>;
      using NT = std::integral_constant<int, (tap + 1) % 9>;
      constexpr bool nload = (tap < 8) || MODE == 0;
      const int npb = (tap < 8) ? pcur : pnext;
      if constexpr (TM == 2) {
        using PN = std::integral_constant<int, 1 - PAR>;
        if constexpr (i < 12) m16_mma(oA[1], oB[1 - PAR], I1{}, PN{}, IC);
        else m16_mma(oA[1], oB[PAR], I1{}, std::integral_constant<int, PAR>{}, std::integral_constant<int, (i - 12) % 12>{});
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (nload) {
          m16_load_slot(oA[0], I1{}, I0{}, NT{}, npb, IC, I0{}, std::integral_constant<int, 8>{},
                        std::integral_constant<int, 2>{});
          m16_load_slot(oB[1 - PAR], I0{}, PN{}, NT{}, npb, IC, std::integral_constant<int, 12>{},
                        std::integral_constant<int, 20>{}, std::integral_constant<int, 2>{});
        }
        issue_at(IC, std::integral_constant<int, 4>{}, std::integral_constant<int, 7>{},
                 std::integral_constant<int, 17>{});
      } else {
        m16_mma(oA[PAR], oB[1], I0{}, I1{}, IC);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (nload) {
          m16_load_slot(oA[1 - PAR], I1{}, I0{}, NT{}, npb, IC, I0{}, std::integral_constant<int, 8>{},
                        std::integral_constant<int, 4>{});
          m16_load_slot(oB[0], I0{}, I0{}, NT{}, npb, IC, std::integral_constant<int, 4>{},
                        std::integral_constant<int, 10>{}, std::integral_constant<int, 4>{});
        }
        issue_at(IC, std::integral_constant<int, 2>{}, std::integral_constant<int, 9>{},
                 std::integral_constant<int, 11>{});
      }
    };
    auto half2 = [&](auto IC) {
      constexpr int i = decltype(IC)::value;
      if constexpr (i < NMMA2) {
        mma_one(f1, IC, std::integral_constant<int, 1>{});
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (i < NRD) {
        if constexpr (tap < 8) read_one(f0, IC, std::integral_constant<int, (tap + 1) % 9>{}, I0{}, pcur);
        else if constexpr (MODE == 0) read_one(f0, IC, I0{}, I0{}, pnext);
        __builtin_amdgcn_sched_barrier(0);
      }
      {
        constexpr int at_patch = (BN == 128) ? 2 : 1, at_b0 = (BN == 128) ? 6 : 4, at_b1 = 10;
        issue_at(IC, std::integral_constant<int, at_patch>{}, std::integral_constant<int, at_b0>{},
                 std::integral_constant<int, at_b1>{});
        if constexpr (PRO && tap == 0 && i == 5) {
          // raw window of the tile after the successor: issued AFTER this stage's weights (so that the waits of the next
          // two stages can leave it in flight), consumed after the K loop
          if (rawfly) fetch_raw(mt_next2);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if constexpr (PRO && i < 6) {
        pro_slot(std::integral_constant<int, (tap % 3) * 12 + 6 + i>{}, std::integral_constant<int, tap / 3>{});
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    if constexpr (M16) {
      pt_unroll(std::make_integer_sequence<int, NSL16>{}, m16_half2);
    } else {
    half2(std::integral_constant<int, 0>{});
    half2(std::integral_constant<int, 1>{});
    half2(std::integral_constant<int, 2>{});
    half2(std::integral_constant<int, 3>{});
    half2(std::integral_constant<int, 4>{});
    half2(std::integral_constant<int, 5>{});
    half2(std::integral_constant<int, 6>{});
    half2(std::integral_constant<int, 7>{});
    half2(std::integral_constant<int, 8>{});
    half2(std::integral_constant<int, 9>{});
    half2(std::integral_constant<int, 10>{});
    half2(std::integral_constant<int, 11>{});
    }
  };
  auto slab_body = [&](auto LASTC, auto PROC, auto SPARC, int slab, int pslab, const u32x4* wb2, int ws2) {
    stage(std::integral_constant<int, 0>{}, LASTC, PROC, SPARC, slab, pslab, wb2, ws2);
    stage(std::integral_constant<int, 1>{}, LASTC, PROC, SPARC, slab, pslab, wb2, ws2);
    stage(std::integral_constant<int, 2>{}, LASTC, PROC, SPARC, slab, pslab, wb2, ws2);
    stage(std::integral_constant<int, 3>{}, LASTC, PROC, SPARC, slab, pslab, wb2, ws2);
    stage(std::integral_constant<int, 4>{}, LASTC, PROC, SPARC, slab, pslab, wb2, ws2);
    stage(std::integral_constant<int, 5>{}, LASTC, PROC, SPARC, slab, pslab, wb2, ws2);
    stage(std::integral_constant<int, 6>{}, LASTC, PROC, SPARC, slab, pslab, wb2, ws2);
    stage(std::integral_constant<int, 7>{}, LASTC, PROC, SPARC, slab, pslab, wb2, ws2);
    stage(std::integral_constant<int, 8>{}, LASTC, PROC, SPARC, slab, pslab, wb2, ws2);
  };
  // slabs 0 .. nslab-2 are interior; the last one is a transition slab when the tile has a successor
  // 8x8-block variants (no LDS room to park a table): chained when the successor works on the same pixel tile
  // (another channel tile of it - the usual order inside an XCD's chunk), whose table is the one in registers
  const bool chain = !FUSE1 && has_next && (STREAM || mt_next == mt);
  if constexpr (OVL) {
    using I1 = std::integral_constant<int, 1>;
    slab_body(I0{}, I0{}, I0{}, 0, 1, wbase, 1);
    pcur = bufY;
    pnext = bufZ;  // the successor's first slab: its first fragments are read at the end of the transition slab
    if (has_next) {
      rawfly = has_next2;
      slab_body(I0{}, I1{}, I0{}, 1, 0, wbase, 0);  // transition slab (same weights for every tile) + the successor's conv1_1
      if (c11max > PT_SAT_FP16) atomicAdd(&rng[2], 1u);
      c11max = 0.f;
    } else {
      rawfly = false;
      slab_body(I1{}, I0{}, I0{}, 1, 0, wbase, 0);
    }
    primed = has_next;
  } else {
  if (chain) wbase_next = wp + (long)(nt_next * BN) * (cin8 * 2);
  if constexpr (M16) {
    // The stage parity continues across slabs (nine stages each): even slabs start with parity 0, odd ones with 1, and
    // a tile has an even number of them (mmmot_patch_m16).  The slabs run in PAIRS, one body of each parity behind the
    // other: a branch between the two bodies inside the loop would keep the accumulators of both alive (scratch).
    using I1 = std::integral_constant<int, 1>;
    auto swap_bufs = [&]() {
      const int t = pcur;
      pcur = pnext;
      pnext = t;
    };
    const int npair = chain ? (nslab >> 1) : (nslab >> 1) - 1;
    for (int slab = 0; slab < 2 * npair; slab += 2) {
      slab_body(I0{}, I0{}, I0{}, slab, slab + 1, wbase, slab + 1);
      swap_bufs();
      const bool trans = (slab + 2 == nslab);
      if constexpr (STREAM) {
        if (trans) {  // the successor's table replaces this tile's, as below
          const unsigned* pk = reinterpret_cast<const unsigned*>(smem + POFF_OFF) + tid;
#pragma unroll
          for (int k = 0; k < G::PA; ++k) poff[k] = pk[k * 512];
        }
      }
      slab_body(I0{}, I0{}, I1{}, slab + 1, trans ? 0 : slab + 2, trans ? wbase_next : wbase, trans ? 0 : slab + 2);
      if (!trans) swap_bufs();
    }
    if (!chain) {
      slab_body(I0{}, I0{}, I0{}, nslab - 2, nslab - 1, wbase, nslab - 1);
      swap_bufs();
      slab_body(I1{}, I0{}, I1{}, nslab - 1, 0, wbase, 0);
    }
  } else {
  const int nloop = chain ? nslab : nslab - 1;
  for (int slab = 0; slab < nloop; ++slab) {
    const bool trans = (slab == nslab - 1);
    if constexpr (STREAM) {
      if (trans) {  // the successor's table replaces this tile's (dead: its last patch slab was requested a slab ago)
        const unsigned* pk = reinterpret_cast<const unsigned*>(smem + POFF_OFF) + tid;
#pragma unroll
        for (int k = 0; k < G::PA; ++k) poff[k] = pk[k * 512];
      }
    }
    slab_body(std::integral_constant<int, 0>{}, I0{}, I0{}, slab, trans ? 0 : slab + 1, trans ? wbase_next : wbase,
              trans ? 0 : slab + 1);
    if (!trans) {
      const int t = pcur;
      pcur = pnext;
      pnext = t;
    }
  }
  if (!chain) slab_body(std::integral_constant<int, 1>{}, I0{}, I0{}, nslab - 1, 0, wbase, 0);
  }
  primed = chain;
  }
