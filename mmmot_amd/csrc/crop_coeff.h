// Device functions shared by the two image resamplers (crop_resize.hip: frame -> S x S crop; crop_augment.hip: region
// of that crop -> S x S training crop): Pillow's triangle-filter coefficients (src/libImaging/Resample.c
// precompute_coeffs + normalize_coeffs_8bpc), its 8-bit clip, and torchvision's to_tensor + normalize of one byte.
#pragma once
#include "common.h"

#define CR_PREC 22

__device__ __forceinline__ double cr_tri(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? __dsub_rn(1.0, x) : 0.0;
}

// Output index xx of an axis that resamples in_size (> 0) input samples to S: bounds[0] = first input sample,
// bounds[1] = number of taps, kk[0 .. kmax) = the 22-bit fixed-point weights (zero behind the taps).  Double precision,
// every operation rounded on its own, as the C code compiled for baseline x86-64.  kmax >= 2*ceil(max(1, in_size/S)) + 1.
__device__ __forceinline__ void cr_coeffs(int in_size, int S, int xx, int kmax, int* bounds, int* kk) {
  const double scale = __ddiv_rn((double)(float)in_size, (double)S);
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = filterscale;  // 1.0 * filterscale
  const double ss = __ddiv_rn(1.0, filterscale);
  const double center = __dmul_rn(__dadd_rn((double)xx, 0.5), scale);  // in0 = 0
  int xmin = (int)__dadd_rn(__dsub_rn(center, support), 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)__dadd_rn(__dadd_rn(center, support), 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) {
    const double w = cr_tri(__dmul_rn(__dadd_rn(__dsub_rn((double)(x + xmin), center), 0.5), ss));
    ww = __dadd_rn(ww, w);
  }
  for (int x = 0; x < xmax; ++x) {
    double w = cr_tri(__dmul_rn(__dadd_rn(__dsub_rn((double)(x + xmin), center), 0.5), ss));
    if (ww != 0.0) w = __ddiv_rn(w, ww);
    kk[x] = (int)__dadd_rn(0.5, __dmul_rn(w, (double)(1 << CR_PREC)));  // triangle weights are >= 0
  }
  for (int x = xmax; x < kmax; ++x) kk[x] = 0;
  bounds[0] = xmin;
  bounds[1] = xmax;
}

__device__ __forceinline__ int cr_clip8(int acc) {
  const int v = acc >> CR_PREC;  // arithmetic shift, like Pillow's lookup on in >> PRECISION_BITS
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// to_tensor (/255) then normalize ((x - mean) / std), IEEE fp32 operations
__device__ __forceinline__ float cr_norm(int v8, float mean, float std) {
  return __fdiv_rn(__fsub_rn(__fdiv_rn((float)v8, 255.f), mean), std);
}
