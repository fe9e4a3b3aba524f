// Gap filling of tracked sequences: one interpolated box for every listed frame a track skipped (see
// include/mmmot_hip.h: mmmot_fill_tracks).
//
// Five launches whatever the number of frames, sequences, tracks or holes:
//   ft_check  one thread per table entry: the shape of seq_start / frame_start (a violation stops the whole call, because
//             every later index is derived from them) and the order of the frame numbers (a violation stops its sequence)
//   ft_succ   one thread per detection: its own frame, the next detection of its ID in its sequence, duplicate IDs
//   ft_count  one workgroup per listed frame: the links that span it, among the detections of the at most max_fill
//             listed frames behind it - a contiguous range of detections
//   ft_scan   one workgroup: the exclusive prefix of the counts, then the status and counters of every sequence
//   ft_fill   one workgroup per listed frame: the same gather; a spanning link's row is its rank by track ID
// Integer atomics only (flags and counters); every output word has one writer, so two calls give the same bits.  The
// arithmetic is fp64 with every product and sum rounded on its own and one rounding to fp32 at the store, as in
// csrc/align_points.hip: plain operators under `#pragma clang fp contract(off)`.
#include "common.h"
#include "track_links.h"  // ft_last_le, ft_check_entry, ft_dup_in_frame, ft_successor: shared with smooth_tracks.hip

#define FT_THREADS 256
#define FT_SCAN_THREADS 1024
#define FT_WT (MMMOT_FILL_MAX + 2)  // row length of wtab: w(n, k) = wtab[n * FT_WT + k]
#define FT_PI 3.141592653589793
#define FT_TWO_PI 6.283185307179586

__global__ __launch_bounds__(FT_THREADS) void ft_check_kernel(const int* __restrict__ frame_start,
                                                              const int* __restrict__ frame_no,
                                                              const int* __restrict__ seq_start, int L, int F, int S,
                                                              int* __restrict__ work, int* __restrict__ info) {
  ft_check_entry(blockIdx.x * FT_THREADS + threadIdx.x, frame_start, frame_no, seq_start, L, F, S, work, info);
}

__global__ __launch_bounds__(FT_THREADS) void ft_succ_kernel(const int* __restrict__ ids,
                                                             const int* __restrict__ frame_start,
                                                             const int* __restrict__ frame_no,
                                                             const int* __restrict__ seq_start, int L, int F, int S,
                                                             int max_fill, int* __restrict__ work,
                                                             int* __restrict__ info) {
  const int i = blockIdx.x * FT_THREADS + threadIdx.x;
  if (i >= L || work[0]) return;
  const int pa = ft_last_le(frame_start, F, i);
  const int s = ft_last_le(seq_start, S, pa);
  const int id = ids[i];
  int sj = -1, sf = -1;
  if (id >= 0) {
    if (ft_dup_in_frame(ids, frame_start, pa, i, id)) atomicOr(&info[4 * s], MMMOT_FILL_EDUP);
    int pb = -1;
    sj = ft_successor(ids, frame_start, pa, seq_start[s + 1], id, pb);
    if (sj >= 0) {
      const long long n = (long long)frame_no[pb] - (long long)frame_no[pa];
      if (n >= 2 && n <= max_fill + 1) {
        sf = pb;
        atomicAdd(&info[4 * s + 2], 1);
      } else if (n > max_fill + 1) {
        atomicAdd(&info[4 * s + 3], 1);
      }
    }
  }
  work[1 + i] = pa;
  work[1 + L + i] = sj;
  work[1 + 2 * (long)L + i] = sf;  // the successor's frame when the link is filled, else -1
}

// the detections of the listed frames behind p that a link spanning p can start in: [lo, frame_start[p])
__device__ __forceinline__ int ft_range_lo(const int* __restrict__ frame_start, const int* __restrict__ frame_no, int p,
                                           int first, int max_fill) {
  int q = p;
  const long long np = frame_no[p];
  while (q > first && np - (long long)frame_no[q - 1] <= max_fill) --q;
  return frame_start[q];
}

__global__ __launch_bounds__(FT_THREADS) void ft_count_kernel(const int* __restrict__ frame_start,
                                                              const int* __restrict__ frame_no,
                                                              const int* __restrict__ seq_start, int L, int S,
                                                              int max_fill, const int* __restrict__ work,
                                                              const int* __restrict__ info,
                                                              int* __restrict__ fill_start) {
  __shared__ int total;
  const int p = blockIdx.x;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  if (!work[0]) {
    const int s = ft_last_le(seq_start, S, p);
    if (info[4 * s] == 0) {
      const int* __restrict__ sf = work + 1 + 2 * (long)L;
      const int lo = ft_range_lo(frame_start, frame_no, p, seq_start[s], max_fill), hi = frame_start[p];
      int n = 0;
      for (int c = lo + threadIdx.x; c < hi; c += FT_THREADS) n += sf[c] > p;
      if (n) atomicAdd(&total, n);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) fill_start[p + 1] = total;
}

__global__ __launch_bounds__(FT_SCAN_THREADS) void ft_scan_kernel(const int* __restrict__ seq_start, int F, int S,
                                                                  int capacity, const int* __restrict__ work,
                                                                  int* __restrict__ fill_start,
                                                                  int* __restrict__ info) {
  __shared__ int part[FT_SCAN_THREADS];
  const int t = threadIdx.x;
  const int chunk = (F + FT_SCAN_THREADS - 1) / FT_SCAN_THREADS;
  const int a = min(t * chunk, F), b = min(a + chunk, F);
  int sum = 0;
  for (int p = a; p < b; ++p) sum += fill_start[p + 1];
  part[t] = sum;
  __syncthreads();
  for (int o = 1; o < FT_SCAN_THREADS; o <<= 1) {
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - sum;
  if (t == 0) fill_start[0] = 0;
  for (int p = a; p < b; ++p) {
    run += fill_start[p + 1];
    fill_start[p + 1] = run;
  }
  __syncthreads();
  const bool bad = work[0] != 0;
  for (int s = t; s < S; s += FT_SCAN_THREADS) {
    int st = info[4 * s] | (bad ? MMMOT_FILL_ECONTRACT : 0);
    int rows = 0, filled = 0, longer = 0;
    if (st == 0) {
      const int end = fill_start[seq_start[s + 1]];
      rows = end - fill_start[seq_start[s]];
      filled = info[4 * s + 2], longer = info[4 * s + 3];
      if (rows > 0 && end > capacity) st = MMMOT_FILL_ECAPACITY;
    }
    info[4 * s] = st, info[4 * s + 1] = rows, info[4 * s + 2] = filled, info[4 * s + 3] = longer;
  }
}

__device__ __forceinline__ double ft_blend(double a, double b, double w1, double w) {
#pragma clang fp contract(off)
  const double u = w1 * a, v = w * b;
  return u + v;
}

// row x 4x4 with the row's fourth entry 1, columns 0..2: ((x*M[0][j] + y*M[1][j]) + z*M[2][j]) + M[3][j]
__device__ __forceinline__ void ft_affine(double& x, double& y, double& z, const double* __restrict__ M) {
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

// into [-pi, pi) by at most four steps of 2 pi
__device__ __forceinline__ double ft_wrap(double d) {
#pragma clang fp contract(off)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (d >= FT_PI) d = d - FT_TWO_PI;
    else if (d < -FT_PI) d = d + FT_TWO_PI;
  }
  return d;
}

__global__ __launch_bounds__(FT_THREADS) void ft_fill_kernel(const float* __restrict__ det, const int* __restrict__ ids,
                                                             const int* __restrict__ frame_start,
                                                             const int* __restrict__ frame_no,
                                                             const int* __restrict__ seq_start,
                                                             const double* __restrict__ xf,
                                                             const double* __restrict__ wtab, int L, int S, int max_fill,
                                                             int capacity, const int* __restrict__ work,
                                                             const int* __restrict__ fill_start,
                                                             const int* __restrict__ info, float* __restrict__ out,
                                                             int* __restrict__ out_id, int* __restrict__ out_src) {
#pragma clang fp contract(off)
  const int p = blockIdx.x;
  if (work[0]) return;
  const int s = ft_last_le(seq_start, S, p);
  if (info[4 * s] & (MMMOT_FILL_EDUP | MMMOT_FILL_ECONTRACT)) return;
  const int row0 = fill_start[p];
  if (fill_start[p + 1] == row0) return;
  const int* __restrict__ own = work + 1;
  const int* __restrict__ sj = work + 1 + L;
  const int* __restrict__ sf = work + 1 + 2 * (long)L;
  const int lo = ft_range_lo(frame_start, frame_no, p, seq_start[s], max_fill), hi = frame_start[p];
  for (int c = lo + threadIdx.x; c < hi; c += FT_THREADS) {
    if (sf[c] <= p) continue;
    const int id = ids[c];
    int rank = 0;
    for (int o = lo; o < hi; ++o) rank += (sf[o] > p && ids[o] < id);
    const long r = (long)row0 + rank;
    if (r >= capacity) continue;
    const int pa = own[c], pb = sf[c], j = sj[c];
    const int n = frame_no[pb] - frame_no[pa], k = frame_no[p] - frame_no[pa];
    const double w = wtab[n * FT_WT + k];
    const double w1 = 1.0 - w;
    const float* __restrict__ a = det + (long)c * 12;
    const float* __restrict__ b = det + (long)j * 12;
    float* __restrict__ o = out + r * 12;
#pragma unroll
    for (int v = 0; v < 7; ++v) o[v] = (float)ft_blend((double)a[v], (double)b[v], w1, w);
    o[11] = (float)ft_blend((double)a[11], (double)b[11], w1, w);
    double bx = (double)b[7], by = (double)b[8], bz = (double)b[9];
    double dyb = 0.0, dyp = 0.0;
    const double* __restrict__ rec_b = nullptr;
    const double* __restrict__ rec_p = nullptr;
    if (xf) {
      rec_b = xf + ((long)pa * (max_fill + 1) + (pb - pa - 1)) * MMMOT_FILL_REC;
      rec_p = xf + ((long)pa * (max_fill + 1) + (p - pa - 1)) * MMMOT_FILL_REC;
      ft_affine(bx, by, bz, rec_b);  // the later observation in the earlier one's coordinates
      dyb = rec_b[32], dyp = rec_p[32];
    }
    double x = ft_blend((double)a[7], bx, w1, w), y = ft_blend((double)a[8], by, w1, w),
           z = ft_blend((double)a[9], bz, w1, w);
    if (xf) ft_affine(x, y, z, rec_p + 16);  // on into the hole frame's coordinates
    o[7] = (float)x, o[8] = (float)y, o[9] = (float)z;
    const double ya = (double)a[10];
    const double yb = (double)b[10] + dyb;
    const double d = ft_wrap(yb - ya);
    const double wd = w * d;
    const double yy = ya + wd;
    o[10] = (float)ft_wrap(yy - dyp);
    out_id[r] = id;
    out_src[2 * r] = c;
    out_src[2 * r + 1] = j;
  }
}

extern "C" int mmmot_fill_tracks(const float* det, const int* ids, const int* frame_start, const int* frame_no,
                                 const int* seq_start, const double* xf, const double* wtab, int L, int F, int S,
                                 int max_fill, int capacity, int* work, int* fill_start, float* out, int* out_id,
                                 int* out_src, int* info, void* stream) {
  if (S < 1 || L < 0 || F < 0 || capacity < 0 || max_fill < 1 || max_fill > MMMOT_FILL_MAX) return MMMOT_EINVAL;
  if (L == 0 || F == 0) return MMMOT_OK;
  if (!det || !ids || !frame_start || !frame_no || !seq_start || !wtab || !work || !fill_start || !info)
    return MMMOT_EINVAL;
  if (capacity > 0 && (!out || !out_id || !out_src)) return MMMOT_EINVAL;
  if ((long)L * 3 + 1 > 0x7fffffffL) return MMMOT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  int rc = mm_check(hipMemsetAsync(work, 0, sizeof(int), st));
  if (rc != MMMOT_OK) return rc;
  rc = mm_check(hipMemsetAsync(info, 0, sizeof(int) * 4 * (size_t)S, st));
  if (rc != MMMOT_OK) return rc;
  const int n_tab = F > S ? F : S;
  hipLaunchKernelGGL(ft_check_kernel, dim3((unsigned)((n_tab + FT_THREADS - 1) / FT_THREADS)), dim3(FT_THREADS), 0, st,
                     frame_start, frame_no, seq_start, L, F, S, work, info);
  hipLaunchKernelGGL(ft_succ_kernel, dim3((unsigned)((L + FT_THREADS - 1) / FT_THREADS)), dim3(FT_THREADS), 0, st, ids,
                     frame_start, frame_no, seq_start, L, F, S, max_fill, work, info);
  hipLaunchKernelGGL(ft_count_kernel, dim3((unsigned)F), dim3(FT_THREADS), 0, st, frame_start, frame_no, seq_start, L, S,
                     max_fill, work, info, fill_start);
  hipLaunchKernelGGL(ft_scan_kernel, dim3(1), dim3(FT_SCAN_THREADS), 0, st, seq_start, F, S, capacity, work, fill_start,
                     info);
  hipLaunchKernelGGL(ft_fill_kernel, dim3((unsigned)F), dim3(FT_THREADS), 0, st, det, ids, frame_start, frame_no,
                     seq_start, xf, wtab, L, S, max_fill, capacity, work, fill_start, info, out, out_id, out_src);
  return mm_check(hipGetLastError());
}
