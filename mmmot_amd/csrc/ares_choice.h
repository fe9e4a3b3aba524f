// Which kernel serves a call of mmmot_gemm_ares (include/mmmot_hip.h): one pure host function, no HIP dependency, so that
// a test can ask it without a GPU (tests/test_ares_choice_cpu.py).  mmmot_gemm_ares (gemm_ares.hip) has checked the
// arguments before it asks: K is 64 or 128, N a multiple of 128 up to 4096, ldx and ldsc multiples of 4.
#pragma once
#include "../../include/mmmot_hip.h"

enum mmmot_ares_kernel {
  ARES_REFUSE = 0,           // no kernel takes the shape: MMMOT_EINVAL
  ARES_STREAMING,            // gemm_ares_kernel<K / 64, mode>: A-resident rows, weights streamed through LDS (gemm_ares.hip)
  ARES_WEIGHT_RESIDENT,      // gemm_wres64_kernel<mode>: K = 64, the whole weight matrix resident in LDS (gemm_wres.hip)
  ARES_INDEPENDENT_WAVE,     // gemm_wres64i_kernel: K = 64 column-sum pass with independent waves (gemm_wres.hip)
  ARES_WEIGHTS_IN_REGISTERS  // gemm_wreg128_kernel: K = 128 column-sum pass, a wave's weights in registers (gemm_wreg.hip)
};

// mode: bit 0 = statistics (part), bit 1 = column sums (colsum).  variant: mmmot_set_gemm_ares_variant - 0 = automatic,
// 1 = the streaming kernel, 2 = the independent-wave / register kernel whenever the layer is eligible, 3 = K = 64: the
// two-barrier weight-resident kernel only (K = 128: as 0).  Results do not depend on the choice, bit for bit.
static inline mmmot_ares_kernel mmmot_ares_choose(const mmmot_gemm_ares_args* a, int mode, int n_cu, int variant) {
  // K = 64 with the whole weight matrix in LDS (N <= 512).  Variant 1 can only keep the streaming kernel where that
  // kernel can run: it walks 256-channel tiles.
  const bool stream_only = variant == 1 && a->N % 256 == 0;
  if (!stream_only && a->K == 64 && a->N <= 512) {
    // column-sum pass: independent waves when every wave gets a run of half tiles (a small launch is better balanced in
    // 128-row tiles over eight waves)
    if (mode == 2 && variant != 3 && (variant == 2 || 2L * a->T >= 4L * 8 * n_cu)) return ARES_INDEPENDENT_WAVE;
    return ARES_WEIGHT_RESIDENT;
  }
  // K = 128 consumer pass: a workgroup owns 512 channels, everything arrives in 16-byte LDS-DMA pieces, and the launch
  // must fill the chip with whole (tile sequence x channel half) groups of 8 workgroups per XCD
  if (variant != 1 && a->K == 128 && mode == 2 && a->N % 512 == 0 && a->N <= 4096 && a->ldx % 4 == 0 && a->ldx >= 128 &&
      a->ldosc % 4 == 0 && a->ldsc % 4 == 0 && !(a->dbias && a->lddb % 4 != 0) &&
      (variant == 2 || (long)a->T * (a->N / 512) >= 2L * n_cu))
    return ARES_WEIGHTS_IN_REGISTERS;
  return a->N % 256 == 0 ? ARES_STREAMING : ARES_REFUSE;
}
