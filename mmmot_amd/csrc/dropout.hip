// nn.Dropout(p) of the LiDAR encoder in training mode (reference modules/point_net.py:28-39: elementwise over points x
// channels, between relu(bn1(conv1(x))) and the per-detection average pool), fused into the two launches that already
// read and write those [P][512] rows - no extra pass over the tensor, no stored mask:
//   * mmmot_segment_mean_dropout      - forward: the pool of mmmot_segment_mean(relu = 1) over the dropped rows;
//   * mmmot_rows_gather_scale_dropout - backward: mmmot_rows_gather_scale times the same mask (csrc/train.hip: one
//                                       kernel template for both);
//   * mmmot_dropout_mask              - the mask itself as bytes (tests; anyone who wants it materialised).
// The mask is a function of (seed, row, channel) alone - csrc/philox.h - so it does not depend on the grid, the tiles or
// the segment layout, and the backward regenerates what the forward used.  One Philox call serves the four consecutive
// channels a lane owns.  Plain fp32, deterministic.
#include "philox.h"
#include "segpool.h"

// The pool of segpool.h - the one behind mmmot_segment_mean - over fp32 rows with sc / sh and ReLU, each row value passed
// through mm_drop4 before it is added.  With threshold = 0 and scale = 1 every term is v * 1: bit for bit
// mmmot_segment_mean(relu = 1), by construction.
__global__ __launch_bounds__(256) void segment_mean_dropout_kernel(
    const float* __restrict__ X, int ldx, int C, const int* __restrict__ seg_start, const int* __restrict__ seg_count,
    const int* __restrict__ seg_group, const float* __restrict__ sc, const float* __restrict__ sh, int ldsc,
    unsigned long long seed, unsigned threshold, float scale, float* __restrict__ out, int ldo) {
  __shared__ __attribute__((aligned(16))) float red[4][256];
  const SegPool k = mm_seg_pool(C, seg_start, seg_count, nullptr, seg_group, true, sc, sh, ldsc);
  auto row = [&](int t) {
    return mm_drop4(mm_seg_row(k, X, ldx, t, 0, true, 1), mm_dropout_words(seed, (unsigned)(k.start + t), k.c),
                    threshold, scale);
  };
  mm_seg_put(k, red, mm_seg_wave_sum(k, row));
  if (k.wave == 0 && k.cv) mm_seg_mean_store(k, red, k.count, out, ldo);
}

extern "C" int mmmot_segment_mean_dropout(const float* X, int ldx, int C, const int* seg_start, const int* seg_count,
                                          const int* seg_group, int nseg, const float* sc, const float* sh, int ldsc,
                                          unsigned long long seed, unsigned threshold, float scale, float* out, int ldo,
                                          void* stream) {
  if (!sc || !mm_seg_args_ok(X, ldx, C, seg_start, seg_count, nseg, sc, sh, ldsc, out, ldo, true)) return MMMOT_EINVAL;
  hipLaunchKernelGGL(segment_mean_dropout_kernel, dim3(nseg, (C + 255) / 256), dim3(256), 0, (hipStream_t)stream, X, ldx,
                     C, seg_start, seg_count, seg_group, sc, sh, ldsc, seed, threshold, scale, out, ldo);
  return mm_check(hipGetLastError());
}

// out[r][c] = keep(r, c) as a byte (1 kept, 0 dropped); a thread writes the four bytes of one Philox call as one word
__global__ __launch_bounds__(256) void dropout_mask_kernel(unsigned long long seed, unsigned threshold, long R, int C,
                                                           unsigned* __restrict__ out) {
  const int C4 = C >> 2;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < R * C4; idx += (long)gridDim.x * 256) {
    const long r = idx / C4;
    const int c = (int)(idx - r * C4) * 4;
    const u32x4 w = mm_dropout_words(seed, (unsigned)r, c);
    unsigned m = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) m |= (w[e] >= threshold ? 1u : 0u) << (8 * e);
    out[idx] = m;
  }
}

extern "C" int mmmot_dropout_mask(unsigned long long seed, unsigned threshold, long R, int C, unsigned char* out,
                                  void* stream) {
  if (!out || R <= 0 || R > 0xFFFFFFFFL || C <= 0 || C % 4 != 0 || !mm_al16(out)) return MMMOT_EINVAL;
  const long n4 = R * (C / 4);
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(mm_grid256(n4)), dim3(256), 0, (hipStream_t)stream, seed, threshold, R, C,
                     reinterpret_cast<unsigned*>(out));
  return mm_check(hipGetLastError());
}
