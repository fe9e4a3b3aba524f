// Ego-motion alignment of extracted LiDAR points: the second frame of a pair moved into the first frame's coordinates
// (see include/mmmot_hip.h: mmmot_align_points).
//
// Replaces align_points (reference utils/data_util.py:512-520 with lidar_to_imu / imu_to_lidar of
// point_cloud/box_np_ops.py:599-611): rows to the IMU frame, a chain of q @ R.T + T steps, rows back to the LiDAR frame.
// One thread per row, 12 or 16 bytes in and out, under a hundred fp64 operations: memory- and latency-bound at the few
// thousand rows of a frame, so nothing here goes beyond adjacent lanes reading adjacent rows.  The arithmetic is fp64 with
// every product and sum rounded on its own (k = 0..3 in order) and ONE rounding to fp32 at the store.  The compiler's
// default contracts a * b + c into an FMA (it does so across __dmul_rn / __dadd_rn as well), so the two arithmetic helpers
// are written with plain operators under `#pragma clang fp contract(off)`: the ISA has v_mul_f64 / v_add_f64 only.
#include "common.h"

#define AP_THREADS 256

// row x 4x4 with the row's fourth entry 1, columns 0..2: ((x*M[0][j] + y*M[1][j]) + z*M[2][j]) + 1*M[3][j]
__device__ __forceinline__ void ap_affine(double& x, double& y, double& z, const double* __restrict__ M) {
#pragma clang fp contract(off)
  double r[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    double s = x * M[0 + j] + y * M[4 + j];
    s = s + z * M[8 + j];
    r[j] = s + M[12 + j];
  }
  x = r[0], y = r[1], z = r[2];
}

// q @ R.T + T: ((x*R[j][0] + y*R[j][1]) + z*R[j][2]) + T[j]; st = 9 doubles of R (row-major) and 3 of T
__device__ __forceinline__ void ap_step(double& x, double& y, double& z, const double* __restrict__ st) {
#pragma clang fp contract(off)
  double r[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    double s = x * st[3 * j + 0] + y * st[3 * j + 1];
    s = s + z * st[3 * j + 2];
    r[j] = s + st[9 + j];
  }
  x = r[0], y = r[1], z = r[2];
}

__global__ __launch_bounds__(AP_THREADS) void ap_align_kernel(const float* __restrict__ pts, int F, int Q, int NS,
                                                              const int* __restrict__ seg_row0,
                                                              const double* __restrict__ xf, int chain,
                                                              float* __restrict__ out, long out_row0, int ldo) {
  const long i = (long)blockIdx.x * AP_THREADS + threadIdx.x;
  if (i >= Q) return;
  // the row's segment: the last s with seg_row0[s] <= i (empty segments share their start with the next one)
  int lo = 0, hi = NS - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg_row0[mid] <= i) lo = mid; else hi = mid - 1;
  }
  const double* __restrict__ rec = xf + (long)lo * MMMOT_ALIGN_REC;
  const float* __restrict__ p = pts + i * F;
  const float fx = p[0], fy = p[1], fz = p[2];
  double x = (double)fx, y = (double)fy, z = (double)fz;
  ap_affine(x, y, z, rec);
  for (int c = 0; c < chain; ++c) ap_step(x, y, z, rec + 16 + 12 * c);
  ap_affine(x, y, z, rec + 16 + 12 * MMMOT_ALIGN_MAX_CHAIN);
  float* __restrict__ o = out + (out_row0 + i) * (long)ldo;
  o[0] = (float)x;
  o[1] = (float)y;
  o[2] = (float)z;
  if (F == 4) o[3] = p[3];  // a float copy of a loaded value: bit for bit, NaN payloads included
}

extern "C" int mmmot_align_points(const float* pts, int F, int Q, int NS, const int* seg_row0, const double* xf,
                                  int chain, float* out, long out_row0, int ldo, void* stream) {
  if ((F != 3 && F != 4) || Q < 0 || NS < 0 || chain < 0 || chain > MMMOT_ALIGN_MAX_CHAIN || out_row0 < 0)
    return MMMOT_EINVAL;
  if (Q == 0) return MMMOT_OK;
  if (!pts || !seg_row0 || !xf || !out || NS < 1 || ldo < F) return MMMOT_EINVAL;
  hipLaunchKernelGGL(ap_align_kernel, dim3((unsigned)(((long)Q + AP_THREADS - 1) / AP_THREADS)), dim3(AP_THREADS), 0,
                     (hipStream_t)stream, pts, F, Q, NS, seg_row0, xf, chain, out, out_row0, ldo);
  return mm_check(hipGetLastError());
}
