// nn.Dropout(p) of the LiDAR encoder in training mode (reference modules/point_net.py:28-39: elementwise over points x
// channels, between relu(bn1(conv1(x))) and the per-detection average pool), fused into the two launches that already
// read and write those [P][512] rows - no extra pass over the tensor, no stored mask:
//   * mmmot_segment_mean_dropout      - forward: the pool of mmmot_segment_mean(relu = 1) over the dropped rows;
//   * mmmot_rows_gather_scale_dropout - backward: mmmot_rows_gather_scale times the same mask;
//   * mmmot_dropout_mask              - the mask itself as bytes (tests; anyone who wants it materialised).
// The mask is a function of (seed, row, channel) alone - csrc/philox.h - so it does not depend on the grid, the tiles or
// the segment layout, and the backward regenerates what the forward used.  One Philox call serves the four consecutive
// channels a lane owns.  Plain fp32, deterministic.
#include "philox.h"

// keep(r, c + e) ? v[e] * scale : 0
__device__ __forceinline__ f32x4 mm_drop4(f32x4 v, u32x4 w, unsigned threshold, float scale) {
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = w[e] >= threshold ? v[e] * scale : 0.f;
  return v;
}

// Decomposition and summation order of segment_mean_kernel (small_kernels.hip): grid = (nseg, ceil(C/256)), 4 waves split
// the rows of the segment, every lane owns 4 consecutive channels, four accumulators over 16-row strides, LDS reduction
// over the waves.  With threshold = 0 and scale = 1 every term is v * 1: bit for bit that kernel with relu = 1.
__global__ __launch_bounds__(256) void segment_mean_dropout_kernel(
    const float* __restrict__ X, int ldx, int C, const int* __restrict__ seg_start, const int* __restrict__ seg_count,
    const int* __restrict__ seg_group, const float* __restrict__ sc, const float* __restrict__ sh, int ldsc,
    unsigned long long seed, unsigned threshold, float scale, float* __restrict__ out, int ldo) {
  __shared__ __attribute__((aligned(16))) float red[4][256];
  const int s = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.y * 256 + lane * 4;
  const bool cv = c < C;
  const int start = seg_start[s], count = seg_count[s];
  const int g = seg_group ? seg_group[s] : 0;
  f32x4 s4 = {1.f, 1.f, 1.f, 1.f}, h4 = {0.f, 0.f, 0.f, 0.f};
  if (cv) {
    s4 = *reinterpret_cast<const f32x4*>(&sc[(long)g * ldsc + c]);
    h4 = *reinterpret_cast<const f32x4*>(&sh[(long)g * ldsc + c]);
  }
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc2 = acc0, acc3 = acc0;
  auto ld = [&](int t) -> f32x4 {
    const long r = (long)start + t;
    f32x4 v = *reinterpret_cast<const f32x4*>(&X[r * ldx + c]);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaxf(fmaf(v[e], s4[e], h4[e]), 0.f);
    return mm_drop4(v, mm_dropout_words(seed, (unsigned)r, c), threshold, scale);
  };
  if (cv) {
    int t = wave;
    for (; t + 12 < count; t += 16) {
      const f32x4 v0 = ld(t), v1 = ld(t + 4), v2 = ld(t + 8), v3 = ld(t + 12);
      acc0 += v0; acc1 += v1; acc2 += v2; acc3 += v3;
    }
    for (; t < count; t += 4) acc0 += ld(t);
  }
  const f32x4 acc = (acc0 + acc1) + (acc2 + acc3);
  *reinterpret_cast<f32x4*>(&red[wave][lane * 4]) = acc;
  __syncthreads();
  if (wave == 0 && cv) {
    f32x4 r = *reinterpret_cast<const f32x4*>(&red[0][lane * 4]);
    r += *reinterpret_cast<const f32x4*>(&red[1][lane * 4]);
    r += *reinterpret_cast<const f32x4*>(&red[2][lane * 4]);
    r += *reinterpret_cast<const f32x4*>(&red[3][lane * 4]);
    const float inv = 1.f / (float)count;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] *= inv;
    *reinterpret_cast<f32x4*>(&out[(long)s * ldo + c]) = r;
  }
}

extern "C" int mmmot_segment_mean_dropout(const float* X, int ldx, int C, const int* seg_start, const int* seg_count,
                                          const int* seg_group, int nseg, const float* sc, const float* sh, int ldsc,
                                          unsigned long long seed, unsigned threshold, float scale, float* out, int ldo,
                                          void* stream) {
  if (!X || !seg_start || !seg_count || !sc || !sh || !out || nseg <= 0 || C <= 0) return MMMOT_EINVAL;
  if (C % 4 != 0 || ldx % 4 != 0 || ldo % 4 != 0 || ldsc % 4 != 0 || ldx < C || ldo < C || ldsc < C) return MMMOT_EINVAL;
  if (!mm_al16(X) || !mm_al16(out) || !mm_al16(sc) || !mm_al16(sh)) return MMMOT_EINVAL;
  hipLaunchKernelGGL(segment_mean_dropout_kernel, dim3(nseg, (C + 255) / 256), dim3(256), 0, (hipStream_t)stream, X, ldx,
                     C, seg_start, seg_count, seg_group, sc, sh, ldsc, seed, threshold, scale, out, ldo);
  return mm_check(hipGetLastError());
}

// X[r][c] = keep(r, c) ? dscale * (S[rowidx[r]][c] * (scale ? scale[rowidx[r]] : 1)) : 0 - the inner product exactly as
// rows_gather_scale_kernel (train.hip) forms it, same grid-stride loop
__global__ __launch_bounds__(256) void rows_gather_scale_dropout_kernel(const float* __restrict__ S, int lds,
                                                                        const int* __restrict__ rowidx,
                                                                        const float* __restrict__ scale,
                                                                        float* __restrict__ X, int ldx, long R, int C,
                                                                        unsigned long long seed, unsigned threshold,
                                                                        float dscale) {
  const int C4 = C >> 2;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < R * C4; idx += (long)gridDim.x * 256) {
    const long r = idx / C4;
    const int c = (int)(idx - r * C4) * 4;
    const int s = rowidx[r];
    f32x4 v = *reinterpret_cast<const f32x4*>(&S[(long)s * lds + c]);
    if (scale) {
      const float f = scale[s];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= f;
    }
    *reinterpret_cast<f32x4*>(&X[r * ldx + c]) = mm_drop4(v, mm_dropout_words(seed, (unsigned)r, c), threshold, dscale);
  }
}

extern "C" int mmmot_rows_gather_scale_dropout(const float* S, int lds, const int* rowidx, const float* scale, float* X,
                                               int ldx, long R, int C, unsigned long long seed, unsigned threshold,
                                               float dscale, void* stream) {
  if (!S || !rowidx || !X || R <= 0 || R > 0xFFFFFFFFL || C <= 0 || C % 4 != 0 || lds % 4 != 0 || ldx % 4 != 0)
    return MMMOT_EINVAL;
  if (lds < C || ldx < C || !mm_al16(S) || !mm_al16(X)) return MMMOT_EINVAL;
  const long n4 = R * (C / 4);
  const int grid = (int)((n4 + 255) / 256 < 8192 ? (n4 + 255) / 256 : 8192);
  hipLaunchKernelGGL(rows_gather_scale_dropout_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, S, lds, rowidx,
                     scale, X, ldx, R, C, seed, threshold, dscale);
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
  const int grid = (int)((n4 + 255) / 256 < 8192 ? (n4 + 255) / 256 : 8192);
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, seed, threshold, R, C,
                     reinterpret_cast<unsigned*>(out));
  return mm_check(hipGetLastError());
}
