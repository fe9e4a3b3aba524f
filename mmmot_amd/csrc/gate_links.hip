// Motion gate of sequence links: a link whose two 3D boxes lie further apart than an object can travel in the elapsed
// frames becomes an absent edge (a quiet NaN) before the solve (see include/mmmot_hip.h: mmmot_gate_links; DESIGN
// section 11, "Sequences: motion gate").
//
// ONE launch whatever the number of blocks, frames and detections: one workgroup of 256 per link block (frame a, frame
// b, link offset).  Frame b's centres, moved into frame a's camera coordinates by the 4x4 of record (a, b - a - 1), and
// its dimensions are staged in LDS once per block, 512 detections at a time, so no frame size is refused; the threads
// then stride over the n_a x (chunk) entries with consecutive lanes on consecutive k, so a wave stores consecutive words
// of a row.  kept[blk] is an integer reduction in LDS with one global writer.  No floating-point atomics: two calls give
// the same bits.  The arithmetic is fp64 with every product and sum rounded on its own, as in csrc/align_points.hip:
// plain operators under `#pragma clang fp contract(off)`.  The kernel is latency- and memory-bound: a few loads, under
// forty fp64 operations and one store per link.
#include "common.h"

#define GL_THREADS 256
#define GL_TILE 512

// row x 4x4 with the row's fourth entry 1, columns 0..2: ((x*M[0][j] + y*M[1][j]) + z*M[2][j]) + M[3][j] (ap_affine)
__device__ __forceinline__ void gl_affine(double& x, double& y, double& z, const double* __restrict__ M) {
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

// max(a, b) <= ratio * min(a, b), written so that a NaN on either side fails
__device__ __forceinline__ bool gl_size_ok(float a, float b, double ratio) {
#pragma clang fp contract(off)
  const bool gt = a > b;
  const double hi = (double)(gt ? a : b), lo = (double)(gt ? b : a);
  const double lim = ratio * lo;
  return hi <= lim;
}

// link / out_link may be the same buffer (every entry is read, then written, by one thread): no __restrict__ on them
__global__ __launch_bounds__(GL_THREADS) void gl_gate_kernel(const float* __restrict__ det,
                                                             const int* __restrict__ frame_start,
                                                             const int* __restrict__ frame_no,
                                                             const int* __restrict__ blocks,
                                                             const double* __restrict__ xf,
                                                             const double* __restrict__ r2tab,
                                                             const double* __restrict__ inv_r2tab, const float* link,
                                                             float* out_link, int* __restrict__ kept, int L, int F,
                                                             int rec_gaps, long n_link, int mode, int max_dt,
                                                             double max_size_ratio, double weight) {
#pragma clang fp contract(off)
  __shared__ double bx[GL_TILE], by[GL_TILE], bz[GL_TILE];
  __shared__ float bd[3][GL_TILE];
  __shared__ int total;
  const int blk = blockIdx.x, tid = threadIdx.x;
  const int a = blocks[4 * (long)blk], b = blocks[4 * (long)blk + 1], off = blocks[4 * (long)blk + 2];
  // the contract, the same for every thread of the workgroup: a broken block gets kept = -1, nothing else of it is touched
  bool broken = a < 0 || b >= F || a >= b || off < 0 || (xf && b - a > rec_gaps);
  int a0 = 0, b0 = 0, na = 0, nb = 0;
  long long dt = 0;
  if (!broken) {
    a0 = frame_start[a], b0 = frame_start[b];
    const int a1 = frame_start[a + 1], b1 = frame_start[b + 1];
    dt = (long long)frame_no[b] - (long long)frame_no[a];
    broken = a0 < 0 || a1 < a0 || a1 > L || b0 < 0 || b1 < b0 || b1 > L || dt <= 0;
    na = a1 - a0, nb = b1 - b0;
    if (!broken) broken = (long)off + (long)na * (long)nb > n_link;
  }
  if (broken) {
    if (tid == 0) kept[blk] = -1;
    return;
  }
  if (tid == 0) total = 0;
  // dt beyond the table: a NaN radius gates every link by the comparison below
  const bool in_tab = dt <= max_dt;
  const double r2 = in_tab ? r2tab[dt] : __builtin_nan("");
  const double inv_r2 = in_tab ? inv_r2tab[dt] : 0.0;
  double C[16];
  if (xf) {
    const double* __restrict__ rec = xf + ((long)a * rec_gaps + (b - a - 1)) * MMMOT_FILL_REC;
#pragma unroll
    for (int i = 0; i < 16; ++i) C[i] = rec[i];
  }
  const float qnan = __builtin_nanf("");
  int n_kept = 0;
  for (int c0 = 0; c0 < nb; c0 += GL_TILE) {
    const int cw = min(GL_TILE, nb - c0);
    __syncthreads();  // the tile's readers of the round before; `total = 0` in the first round
    for (int k = tid; k < cw; k += GL_THREADS) {
      const float* __restrict__ d = det + (long)(b0 + c0 + k) * 12;
      double x = (double)d[7], y = (double)d[8], z = (double)d[9];
      if (xf) gl_affine(x, y, z, C);
      bx[k] = x, by[k] = y, bz[k] = z;
      bd[0][k] = d[4], bd[1][k] = d[5], bd[2][k] = d[6];
    }
    __syncthreads();
    const long n_ent = (long)na * cw;
    for (long e = tid; e < n_ent; e += GL_THREADS) {
      const int j = (int)(e / cw), k = (int)(e - (long)j * cw);
      const float* __restrict__ d = det + (long)(a0 + j) * 12;
      const double dx = (double)d[7] - bx[k], dy = (double)d[8] - by[k], dz = (double)d[9] - bz[k];
      const double xx = dx * dx, zz = dz * dz;
      double d2 = xx + zz;
      if (mode == 1) {
        const double yy = dy * dy;
        d2 = d2 + yy;
      }
      bool pass = d2 <= r2;  // false for a NaN on either side
      if (max_size_ratio > 0.0)
        pass = pass && gl_size_ok(d[4], bd[0][k], max_size_ratio) && gl_size_ok(d[5], bd[1][k], max_size_ratio) &&
               gl_size_ok(d[6], bd[2][k], max_size_ratio);
      if (!link) {
        n_kept += pass;
        continue;
      }
      const long w = (long)off + (long)j * nb + c0 + k;
      float s = link[w];
      if (!pass) {
        s = qnan;
      } else if (s == s) {
        ++n_kept;
        if (weight > 0.0) {
          const double t = d2 * inv_r2;
          const double u = weight * t;
          const double v = (double)s - u;
          s = (float)v;
        }
      }
      out_link[w] = s;  // a passing score with weight == 0, and a NaN input, go through as loaded: bit for bit
    }
  }
  if (n_kept) atomicAdd(&total, n_kept);
  __syncthreads();
  if (tid == 0) kept[blk] = total;
}

extern "C" int mmmot_gate_links(const float* det, const int* frame_start, const int* frame_no, const int* blocks,
                                const double* xf, const double* r2, const double* inv_r2, const float* link,
                                float* out_link, int* kept, int L, int F, int NB, int rec_gaps, long n_link, int mode,
                                int max_dt, double max_size_ratio, double weight, void* hip_stream) {
  if (NB < 0 || L < 0 || F < 0 || n_link < 0 || max_dt < 1 || max_dt > MMMOT_GATE_MAX_DT || (mode != 0 && mode != 1))
    return MMMOT_EINVAL;
  if (!(max_size_ratio >= 0.0) || !(weight >= 0.0)) return MMMOT_EINVAL;  // NaN included
  if ((link == nullptr) != (out_link == nullptr)) return MMMOT_EINVAL;
  if (xf && rec_gaps < 1) return MMMOT_EINVAL;
  if (NB == 0) return MMMOT_OK;
  if ((L > 0 && !det) || !frame_start || !frame_no || !blocks || !r2 || !inv_r2 || !kept) return MMMOT_EINVAL;
  hipLaunchKernelGGL(gl_gate_kernel, dim3((unsigned)NB), dim3(GL_THREADS), 0, (hipStream_t)hip_stream, det, frame_start,
                     frame_no, blocks, xf, r2, inv_r2, link, out_link, kept, L, F, rec_gaps, n_link, mode, max_dt,
                     max_size_ratio, weight);
  return mm_check(hipGetLastError());
}
