// What the strided segment pools share (segment_mean_kernel in small_kernels.hip, segment_mean_dropout_kernel in
// dropout.hip, segment_argmax_kernel in backward.hip): the segment context, the row value a(t), the wave's walk over a
// segment and the combine of the four waves.  grid = (nseg, ceil(C/256)), 256 threads: the 4 waves split the rows of the
// segment (wave w takes t = w, w + 4, ...), every lane owns 4 consecutive channels (1 KiB per wave load).  "The dropout
// pool with nothing dropped is the plain pool" and "the arg-max row holds the value the forward wrote" hold bit for bit
// because the pieces below exist once.
#pragma once
#include "common.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));

// ---- segment context: block -> segment s, lane -> channels c .. c + 3, the segment's rows and its group's affine ----
struct SegPool {
  int s, lane, wave, c;
  bool cv;  // c < C: the lane has channels
  int start, count, stride;
  f32x4 s4, h4;  // sc / sh of the group at the lane's channels; (1, 0) without a normalisation
};

// `norm`: sc / sh are given (a literal where the entry point requires them)
__device__ __forceinline__ SegPool mm_seg_pool(int C, const int* __restrict__ seg_start, const int* __restrict__ seg_count,
                                               const int* __restrict__ seg_stride, const int* __restrict__ seg_group,
                                               bool norm, const float* __restrict__ sc, const float* __restrict__ sh,
                                               int ldsc) {
  SegPool k;
  k.s = blockIdx.x;
  k.lane = threadIdx.x & 63;
  k.wave = threadIdx.x >> 6;
  k.c = blockIdx.y * 256 + k.lane * 4;
  k.cv = k.c < C;
  k.start = seg_start[k.s];
  k.count = seg_count[k.s];
  k.stride = seg_stride ? seg_stride[k.s] : 1;
  const int g = seg_group ? seg_group[k.s] : 0;
  k.s4 = f32x4{1.f, 1.f, 1.f, 1.f};
  k.h4 = f32x4{0.f, 0.f, 0.f, 0.f};
  if (norm && k.cv) {
    k.s4 = *reinterpret_cast<const f32x4*>(&sc[(long)g * ldsc + k.c]);
    k.h4 = *reinterpret_cast<const f32x4*>(&sh[(long)g * ldsc + k.c]);
  }
  return k;
}

// ---- row value: THE definition of a(t), the lane's four values of row t of the segment ----
// fmt: 0 fp32 rows, 1 hl16 rows, 2 hq8 rows; then fmaf(v, s, h) when `norm`, then fmaxf(., 0) when `relu`.  The address is
// an INDEX into X (uniform row offset + c), not a row pointer carried along: with the pointer form the 16-row loop kept
// sixteen 64-bit per-lane pointers and added to each of them every trip (profiles/README.md)
__device__ __forceinline__ f32x4 mm_seg_row(const SegPool& k, const float* __restrict__ X, int ldx, int t, int fmt,
                                            bool norm, int relu) {
  const long off = ((long)k.start + (long)t * k.stride) * ldx;  // the row, in floats
  const int c = k.c;
  f32x4 v;
  if (fmt == 2) {
    // hq8 row: 128-byte record per 32 channels = [32 x fp16 hi | 32 x e4m3 (unused here) | 32 x e4m3(lo * 2^9)]
    const unsigned char* rec = reinterpret_cast<const unsigned char*>(X + off) + (c >> 5) * 128;
    const f16x4 h = *reinterpret_cast<const f16x4*>(rec + 2 * (c & 31));
    const int l = *reinterpret_cast<const int*>(rec + 96 + (c & 31));
    const auto p0 = __builtin_amdgcn_cvt_pk_f32_fp8(l, false);
    const auto p1 = __builtin_amdgcn_cvt_pk_f32_fp8(l, true);
    v[0] = (float)h[0] + p0[0] * (1.f / 512.f);
    v[1] = (float)h[1] + p0[1] * (1.f / 512.f);
    v[2] = (float)h[2] + p1[0] * (1.f / 512.f);
    v[3] = (float)h[3] + p1[1] * (1.f / 512.f);
  } else if (fmt) {
    // hl16 row (same bytes as fp32): unit u = c>>3 holds [hi8 | lo8] halves; this lane's 4 channels
    const _Float16* rowp = reinterpret_cast<const _Float16*>(X + off);
    const f16x4 h = *reinterpret_cast<const f16x4*>(rowp + (c >> 3) * 16 + (c & 7));
    const f16x4 l = *reinterpret_cast<const f16x4*>(rowp + (c >> 3) * 16 + 8 + (c & 7));
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = mm_hl_join(h[e], l[e]);
  } else {
    v = *reinterpret_cast<const f32x4*>(&X[off + c]);
  }
  if (norm) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaf(v[e], k.s4[e], k.h4[e]);
  }
  if (relu) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
  }
  return v;
}

__device__ __forceinline__ f32x4 mm_max4(f32x4 a, f32x4 b) {
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = fmaxf(a[e], b[e]);
  return r;
}

// a wave's partial in LDS at the lane's channels
__device__ __forceinline__ f32x4& mm_seg_red(float (*red)[256], int wave, const SegPool& k) {
  return *reinterpret_cast<f32x4*>(&red[wave][k.lane * 4]);
}

// ---- mean: the wave's sum of row(t) over its rows - four accumulators over 16-row strides, the tail into the first ----
template <class Row>
__device__ __forceinline__ f32x4 mm_seg_wave_sum(const SegPool& k, Row row) {
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc2 = acc0, acc3 = acc0;
  if (k.cv) {
    int t = k.wave;
    for (; t + 12 < k.count; t += 16) {
      const f32x4 v0 = row(t), v1 = row(t + 4), v2 = row(t + 8), v3 = row(t + 12);
      acc0 += v0; acc1 += v1; acc2 += v2; acc3 += v3;
    }
    for (; t < k.count; t += 4) acc0 += row(t);
  }
  return (acc0 + acc1) + (acc2 + acc3);
}

// a wave's partial -> LDS, then the workgroup barrier; what wave 0 reads back (cv lanes) is combined by the two below
__device__ __forceinline__ void mm_seg_put(const SegPool& k, float (*red)[256], f32x4 acc) {
  mm_seg_red(red, k.wave, k) = acc;
  __syncthreads();
}

__device__ __forceinline__ f32x4 mm_seg_sum_waves(const SegPool& k, float (*red)[256]) {  // in wave order
  f32x4 r = mm_seg_red(red, 0, k);
  r += mm_seg_red(red, 1, k);
  r += mm_seg_red(red, 2, k);
  r += mm_seg_red(red, 3, k);
  return r;
}

// wave 0 after mm_seg_put: the mean = the waves' sums added in wave order times 1 / div -> out[s][c .. c + 3]
__device__ __forceinline__ void mm_seg_mean_store(const SegPool& k, float (*red)[256], int div, float* __restrict__ out,
                                                  int ldo) {
  f32x4 r = mm_seg_sum_waves(k, red);
  const float inv = 1.f / (float)div;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] *= inv;
  *reinterpret_cast<f32x4*>(&out[(long)k.s * ldo + k.c]) = r;
}

// ---- max: the wave's maximum of row(t) (a wave without rows carries -3e38), the waves combined pairwise ----
template <class Row>
__device__ __forceinline__ f32x4 mm_seg_wave_max(const SegPool& k, Row row) {
  f32x4 acc = {-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};
  if (k.cv)
    for (int t = k.wave; t < k.count; t += 4) acc = mm_max4(acc, row(t));
  return acc;
}

__device__ __forceinline__ f32x4 mm_seg_max_waves(const SegPool& k, float (*red)[256]) {
  return mm_max4(mm_max4(mm_seg_red(red, 0, k), mm_seg_red(red, 1, k)), mm_max4(mm_seg_red(red, 2, k), mm_seg_red(red, 3, k)));
}

// ---- arg-max: idx = min { t : a(t) = max_u a(u) }.  A wave keeps (value, index) with a strict > over its increasing t;
// the waves are combined on (larger value, then LOWER INDEX) - not the lower wave: rows 1 and 4 sit in waves 1 and 0.  A
// wave without rows (count < 4) carries index -1 and never enters the combine; wave 0 holds row 0 (count >= 1 is the
// caller's to guarantee, as for the mean). ----
template <class Row>
__device__ __forceinline__ void mm_seg_argmax_store(const SegPool& k, Row row, float (*redv)[256], int (*redi)[256],
                                                    int* __restrict__ idx_out, int ldo) {
  f32x4 best = {0.f, 0.f, 0.f, 0.f};
  i32x4 bi = {-1, -1, -1, -1};
  if (k.cv && k.wave < k.count) {
    best = row(k.wave);
    bi = i32x4{k.wave, k.wave, k.wave, k.wave};
    for (int t = k.wave + 4; t < k.count; t += 4) {
      const f32x4 v = row(t);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (v[e] > best[e]) {
          best[e] = v[e];
          bi[e] = t;
        }
    }
  }
  mm_seg_red(redv, k.wave, k) = best;
  *reinterpret_cast<i32x4*>(&redi[k.wave][k.lane * 4]) = bi;
  __syncthreads();
  if (k.wave == 0 && k.cv) {
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const f32x4 v = mm_seg_red(redv, w, k);
      const i32x4 q = *reinterpret_cast<const i32x4*>(&redi[w][k.lane * 4]);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (q[e] >= 0 && (v[e] > best[e] || (v[e] == best[e] && q[e] < bi[e]))) {
          best[e] = v[e];
          bi[e] = q[e];
        }
    }
    *reinterpret_cast<i32x4*>(&idx_out[(long)k.s * ldo + k.c]) = bi;
  }
}

// ---- host: the argument contract the three pool launchers share.  `ld_at_least_C`: also refuse ldx / ldo / ldsc < C
// (mmmot_segment_mean never has, and must go on accepting what it accepts) ----
static inline bool mm_seg_args_ok(const void* X, int ldx, int C, const int* seg_start, const int* seg_count, int nseg,
                                  const float* sc, const float* sh, int ldsc, const void* out, int ldo,
                                  bool ld_at_least_C) {
  if (!X || !seg_start || !seg_count || !out || nseg <= 0 || C <= 0) return false;
  if (C % 4 != 0 || ldx % 4 != 0 || ldo % 4 != 0 || !mm_al16(X) || !mm_al16(out)) return false;
  if (ld_at_least_C && (ldx < C || ldo < C)) return false;
  if ((sc == nullptr) != (sh == nullptr)) return false;
  if (sc && (ldsc % 4 != 0 || (ld_at_least_C && ldsc < C) || !mm_al16(sc) || !mm_al16(sh))) return false;
  return true;
}
