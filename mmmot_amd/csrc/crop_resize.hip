// Per-detection image preparation on the device: crop (zero padding outside the frame) -> antialiased
// bilinear resize to S x S -> to_tensor -> normalize, i.e. the model input ``dets`` [N][3][S][S]
// (see include/mmmot_hip.h: mmmot_crop_resize_norm).
//
// Replaces, per detection, PIL ``img.crop(box).resize((S, S), Image.BILINEAR)`` + torchvision ToTensor /
// Normalize (reference dataset/test_seq_dataset.py:212-218, utils/build_util.py:111-112,137-142).  The
// arithmetic is Pillow's (src/libImaging/Resample.c): triangle filter with the support stretched by the scale
// when shrinking, coefficients in double precision (every operation rounded on its own, as the C code
// compiled for baseline x86-64), normalised, 22-bit fixed point, two separable passes with an 8-bit
// intermediate - so the uint8 result and the float32 tensor are bit-identical to the reference pipeline.
// Byte work, HBM-bound on the float32 output (3*S*S*4 B per detection); crops are read through L2.
#include "crop_coeff.h"  // cr_tri, cr_coeffs, cr_clip8, cr_norm: shared with crop_augment.hip

// grid (N, 2): axis 0 = horizontal (crop width), 1 = vertical (crop height); thread = output index.
// work layout per (n, axis): bounds [S][2] ints, then kk [S][kmax] ints.
__global__ void cr_coeff_kernel(const int* __restrict__ boxes, int S, int kmax, int* __restrict__ work) {
  const int n = blockIdx.x, axis = blockIdx.y;
  const int xx = blockIdx.z * blockDim.x + threadIdx.x;
  if (xx >= S) return;
  const int* b = boxes + n * 4;
  const int in_size = axis == 0 ? b[2] - b[0] : b[3] - b[1];
  int* base = work + ((long)n * 2 + axis) * S * (2 + kmax);
  int* bounds = base + xx * 2;
  int* kk = base + S * 2 + xx * kmax;
  if (in_size <= 0) {
    bounds[0] = 0;
    bounds[1] = 0;
    return;
  }
  cr_coeffs(in_size, S, xx, kmax, bounds, kk);
}

// output pixel (oy, ox) of crop n from the image img [H][W][3] whose rows lie `pitch` bytes apart: the body of both
// resize kernels
__device__ __forceinline__ void cr_resize_pixel(const unsigned char* __restrict__ img, int H, int W, long pitch,
                                                const int* __restrict__ boxes, int n, int oy, int ox, int S, int kmax,
                                                const int* __restrict__ work, const float* __restrict__ ms,
                                                float* __restrict__ out, unsigned char* __restrict__ out_u8) {
  const int* b = boxes + n * 4;
  const int x1 = b[0], y1 = b[1];
  const int* hb = work + ((long)n * 2 + 0) * S * (2 + kmax);
  const int* vb = work + ((long)n * 2 + 1) * S * (2 + kmax);
  const int xmin = hb[ox * 2], xcnt = hb[ox * 2 + 1];
  const int ymin = vb[oy * 2], ycnt = vb[oy * 2 + 1];
  const int* kh = hb + S * 2 + ox * kmax;
  const int* kv = vb + S * 2 + oy * kmax;
  int acc[3] = {1 << (CR_PREC - 1), 1 << (CR_PREC - 1), 1 << (CR_PREC - 1)};
  for (int j = 0; j < ycnt; ++j) {
    const int gy = y1 + ymin + j;
    int h[3] = {1 << (CR_PREC - 1), 1 << (CR_PREC - 1), 1 << (CR_PREC - 1)};
    if (gy >= 0 && gy < H) {
      const unsigned char* row = img + (long)gy * pitch;
      for (int i = 0; i < xcnt; ++i) {
        const int gx = x1 + xmin + i;
        if (gx >= 0 && gx < W) {
          const int k = kh[i];
          h[0] += row[gx * 3 + 0] * k;
          h[1] += row[gx * 3 + 1] * k;
          h[2] += row[gx * 3 + 2] * k;
        }
      }
    }
    const int k = kv[j];
    acc[0] += cr_clip8(h[0]) * k;  // the 8-bit intermediate image of the two-pass resize
    acc[1] += cr_clip8(h[1]) * k;
    acc[2] += cr_clip8(h[2]) * k;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int v8 = cr_clip8(acc[c]);
    if (out_u8) out_u8[(((long)n * S + oy) * S + ox) * 3 + c] = (unsigned char)v8;
    if (out) {
      out[(((long)n * 3 + c) * S + oy) * S + ox] = cr_norm(v8, ms[c], ms[3 + c]);  // to_tensor, normalize
    }
  }
}

// grid (N, S): one output row per workgroup, one output column per thread.
__global__ __launch_bounds__(256) void cr_resize_kernel(const unsigned char* __restrict__ img, int H, int W,
                                                        const int* __restrict__ boxes, int S, int kmax,
                                                        const int* __restrict__ work, const float* __restrict__ ms,
                                                        float* __restrict__ out, unsigned char* __restrict__ out_u8) {
  const int n = blockIdx.x, oy = blockIdx.y, ox = threadIdx.x;
  if (ox >= S) return;
  cr_resize_pixel(img, H, W, (long)W * 3, boxes, n, oy, ox, S, kmax, work, ms, out, out_u8);
}

// the same grid over the crops of NI images: crop n reads row img_of[n] of the image table [NI][4] = (address, H, W,
// row pitch in bytes); a crop whose index lies outside [0, NI) is skipped (nothing of it is written)
__global__ __launch_bounds__(256) void cr_resize_multi_kernel(const long long* __restrict__ images, int NI,
                                                              const int* __restrict__ img_of,
                                                              const int* __restrict__ boxes, int S, int kmax,
                                                              const int* __restrict__ work,
                                                              const float* __restrict__ ms, float* __restrict__ out,
                                                              unsigned char* __restrict__ out_u8) {
  const int n = blockIdx.x, oy = blockIdx.y, ox = threadIdx.x;
  const int im = img_of[n];
  if (ox >= S || im < 0 || im >= NI) return;
  const long long* e = images + 4 * (long)im;
  cr_resize_pixel((const unsigned char*)e[0], (int)e[1], (int)e[2], (long)e[3], boxes, n, oy, ox, S, kmax, work, ms, out,
                  out_u8);
}

extern "C" int mmmot_crop_resize_norm_multi(const long long* images, int NI, const int* img_of, const int* boxes, int N,
                                            int S, int kmax, const float* mean_std, int* work, float* out,
                                            unsigned char* out_u8, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) return 0;
  if (!images || !img_of || !boxes || !mean_std || !work || (!out && !out_u8) || NI < 1 || N < 0) return MMMOT_EINVAL;
  if (S <= 0 || S > 256 || kmax < 3) return MMMOT_EINVAL;
  hipLaunchKernelGGL(cr_coeff_kernel, dim3(N, 2, (S + 63) / 64), dim3(64), 0, s, boxes, S, kmax, work);
  hipLaunchKernelGGL(cr_resize_multi_kernel, dim3(N, S), dim3(256), 0, s, images, NI, img_of, boxes, S, kmax, work,
                     mean_std, out, out_u8);
  return mm_check(hipGetLastError());
}

extern "C" int mmmot_crop_resize_norm(const unsigned char* img, int H, int W, const int* boxes, int N, int S, int kmax,
                                      const float* mean_std, int* work, float* out, unsigned char* out_u8,
                                      void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!img || !boxes || !mean_std || !work || (!out && !out_u8) || H <= 0 || W <= 0 || N <= 0) return MMMOT_EINVAL;
  if (S <= 0 || S > 256 || kmax < 3) return MMMOT_EINVAL;
  hipLaunchKernelGGL(cr_coeff_kernel, dim3(N, 2, (S + 63) / 64), dim3(64), 0, s, boxes, S, kmax, work);
  hipLaunchKernelGGL(cr_resize_kernel, dim3(N, S), dim3(256), 0, s, img, H, W, boxes, S, kmax, work, mean_std, out,
                     out_u8);
  return mm_check(hipGetLastError());
}

// ToTensor + Normalize of 8-bit crops [N][S][S][3] -> fp32 [N][3][S][S] (the same IEEE divisions as cr_resize_kernel):
// the model input for the paths that cannot take the bytes directly (exact-fp32 trunk, unfused first layer).
__global__ __launch_bounds__(256) void cr_u8_normalize_kernel(const unsigned char* __restrict__ u8, long npix, int S2,
                                                               const float* __restrict__ ms, float* __restrict__ out) {
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const long n = p / S2;
    const int r = (int)(p - n * S2);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      out[(n * 3 + c) * S2 + r] = cr_norm(u8[p * 3 + c], ms[c], ms[3 + c]);
    }
  }
}

extern "C" int mmmot_u8_normalize(const unsigned char* u8, int N, int S, const float* mean_std, float* out, void* stream) {
  if (!u8 || !mean_std || !out || N <= 0 || S <= 0) return MMMOT_EINVAL;
  const long npix = (long)N * S * S;
  hipLaunchKernelGGL(cr_u8_normalize_kernel, dim3(mm_grid256(npix)), dim3(256), 0, (hipStream_t)stream, u8, npix, S * S, mean_std, out);
  return mm_check(hipGetLastError());
}
