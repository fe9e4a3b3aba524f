// Training labels on the device (include/mmmot_hip.h: mmmot_generate_gt, mmmot_match_dets).
//
// mmmot_generate_gt restates TrackingModule.generate_gt (reference tracking_model.py:294-351), mmmot_match_dets restates
// generate_det_id_matrix (reference dataset/common.py:82-111) - both literally, quirks included.
// Neither is arithmetic or bandwidth work: the point is one launch per sample and no host loop.  One workgroup of four
// waves serves a chain (a frame); everything it compares sits in LDS; every output element is written exactly once, by a
// plain store of the lane that owns it - no atomics on global memory, no read-modify-write, so the results do not
// depend on the chain's (frame's) place in the batch.
//
// The fp64 distance of mmmot_match_dets is one IEEE operation per step: no contraction into FMAs in this file.
#pragma clang fp contract(off)
#include "common.h"

#define LB_THREADS 256
#define LB_MAXT MMMOT_CHAIN_MAXT
#define LB_ROW MMMOT_CHAIN_ROW
#define LB_MAXN 512
#define LB_MAXL 1024

__global__ __launch_bounds__(LB_THREADS) void generate_gt_kernel(const int* __restrict__ ids, const int* __restrict__ cls,
                                                                  const int* __restrict__ chains, int max_n, int cap,
                                                                  float* __restrict__ out,
                                                                  const int* __restrict__ out_off) {
  __shared__ int s_id[LB_MAXL], s_cls[LB_MAXL], s_succ[LB_MAXL];
  __shared__ int s_st[LB_MAXT + 1];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int* ch = chains + LB_ROW * p;
  const int T = ch[0], so = ch[1];
  bool ok = T >= 2 && T <= LB_MAXT && so >= 0;
  int L = 0;
  if (ok) {
    for (int t = 0; t < T; ++t) {
      const int n = ch[3 + t];
      ok = ok && n >= 0 && n <= max_n && n <= LB_MAXN;
      L += ok ? n : 0;
    }
  }
  float* o = out + out_off[p];
  if (!ok || L < 1 || L > cap || L > LB_MAXL) {  // outside the launch's contract: the marker and nothing else
    if (tid == 0) o[0] = __builtin_nanf("");
    return;
  }
  if (tid == 0) {
    int a = 0;
    for (int t = 0; t < T; ++t) {
      s_st[t] = a;
      a += ch[3 + t];
    }
    s_st[T] = a;
  }
  for (int v = tid; v < L; v += LB_THREADS) {
    s_id[v] = ids[so + v];
    s_cls[v] = cls[so + v];
  }
  __syncthreads();

  // per detection: gt_det / gt_new / gt_end and its successor (the first equal id of the next frame; -1: none, or the
  // detection is not a positive one and links nothing)
  for (int v = tid; v < L; v += LB_THREADS) {
    int t = 0;
    while (s_st[t + 1] <= v) ++t;  // s_st[T] = L > v: ends at t <= T - 1 (empty frames are stepped over)
    const bool pos = s_cls[v] == 1;
    const int id = s_id[v];
    int succ = -1;
    bool prev = false;
    if (pos) {
      if (t < T - 1) {
        const int a = s_st[t + 1], n = s_st[t + 2] - a;
        for (int k = 0; k < n; ++k)
          if (s_id[a + k] == id) {
            succ = k;
            break;
          }
      }
      if (t > 0) {
        const int a = s_st[t - 1], n = s_st[t] - a;
        for (int k = 0; k < n; ++k)
          if (s_id[a + k] == id) {
            prev = true;
            break;
          }
      }
    }
    s_succ[v] = succ;
    o[v] = pos ? 1.f : 0.f;
    o[L + v] = pos && !prev ? 1.f : 0.f;
    o[2 * L + v] = pos && succ < 0 ? 1.f : 0.f;
  }
  __syncthreads();

  // link blocks: a wave per row j, its lanes over the row's n_{t+1} elements
  int lo = 3 * L;
  for (int t = 0; t < T - 1; ++t) {
    const int a = s_st[t], n0 = s_st[t + 1] - a, n1 = s_st[t + 2] - s_st[t + 1];
    for (int j = wv; j < n0; j += LB_THREADS / 64) {
      const int succ = s_succ[a + j];
      float* row = o + lo + j * n1;
      for (int k = lane; k < n1; k += 64) row[k] = k == succ ? 1.f : 0.f;
    }
    lo += n0 * n1;
  }
}

extern "C" int mmmot_generate_gt(const int* ids, const int* cls, const int* chains, int B, int max_n, int max_L,
                                 float* out, const int* out_off, void* stream) {
  if (!ids || !cls || !chains || !out || !out_off) return MMMOT_EINVAL;
  if (B < 1 || max_n < 1 || max_n > LB_MAXN || max_L < 1 || max_L > LB_MAXL || max_n > max_L) return MMMOT_EINVAL;
  if ((long)max_L > (long)LB_MAXT * max_n) return MMMOT_EINVAL;  // at most 8 frames of at most max_n each
  hipLaunchKernelGGL(generate_gt_kernel, dim3(B), dim3(LB_THREADS), 0, (hipStream_t)stream, ids, cls, chains, max_n,
                     max_L, out, out_off);
  return mm_check(hipGetLastError());
}

// ---- detections -> ground-truth identities ----------------------------------------------------------------------------
// 1 - IoU of two x, y, w, h boxes as the reference's distance matrix holds it after ``mat[isnan] = 10`` and
// ``torch.Tensor(mat)``: fp64, one operation per step, rounded to fp32 once at the end
__device__ __forceinline__ float lb_dist(double gx, double gy, double gw, double gh, double dx, double dy, double dw,
                                         double dh, double max_iou) {
  const double gbx = gx + gw, gby = gy + gh, dbx = dx + dw, dby = dy + dh;
  const double ix = fmax(fmin(gbx, dbx) - fmax(gx, dx), 0.0);
  const double iy = fmax(fmin(gby, dby) - fmax(gy, dy), 0.0);
  const double isect = ix * iy;
  const double ag = gw * gh, ad = dw * dh;
  const double uni = ag + ad - isect;
  if (uni == 0.0) return 10.f;
  const double dist = 1.0 - isect / uni;
  if (!(dist <= max_iou)) return 10.f;  // above the gate, or NaN
  return (float)dist;
}

__global__ __launch_bounds__(LB_THREADS) void match_dets_kernel(const double* __restrict__ det, const double* __restrict__ gt,
                                                                 const int* __restrict__ gt_id,
                                                                 const int* __restrict__ gt_name,
                                                                 const int* __restrict__ frames, int car_code,
                                                                 int dontcare_code, double max_iou, int max_n,
                                                                 int* __restrict__ det_id, int* __restrict__ det_cls) {
  __shared__ double s_box[LB_MAXN * 4];
  __shared__ int s_win[LB_MAXN];
  const int f = blockIdx.x, tid = threadIdx.x;
  const int doff = frames[4 * f], nd = frames[4 * f + 1], goff = frames[4 * f + 2], ng = frames[4 * f + 3];
  if (doff < 0 || goff < 0 || nd < 1 || ng < 0 || nd > max_n || ng > max_n || nd > LB_MAXN || ng > LB_MAXN)
    return;  // no detection to label, or a frame outside the launch's contract: nothing of it is written
  for (int e = tid; e < 4 * nd; e += LB_THREADS) s_box[e] = det[4 * (long)doff + e];
  for (int d = tid; d < nd; d += LB_THREADS) s_win[d] = -1;
  __syncthreads();
  for (int i = tid; i < ng; i += LB_THREADS) {
    const double* g = gt + 4 * (long)(goff + i);
    const double gx = g[0], gy = g[1], gw = g[2], gh = g[3];
    float best = lb_dist(gx, gy, gw, gh, s_box[0], s_box[1], s_box[2], s_box[3], max_iou);
    int arg = 0;
    for (int d = 1; d < nd; ++d) {
      const float v = lb_dist(gx, gy, gw, gh, s_box[4 * d], s_box[4 * d + 1], s_box[4 * d + 2], s_box[4 * d + 3], max_iou);
      if (v < best) {  // ties stay with the smallest index
        best = v;
        arg = d;
      }
    }
    atomicMax(&s_win[arg], i);  // LDS: the reference's loop overwrites in the order of i, so the largest i stays
  }
  __syncthreads();
  for (int d = tid; d < nd; d += LB_THREADS) {
    const int w = s_win[d];
    int id = -1, c = 0;
    if (w >= 0) {
      id = gt_id[goff + w];
      const int name = gt_name[goff + w];
      c = name == car_code ? 1 : (name == dontcare_code ? -1 : 0);
    }
    det_id[doff + d] = id;
    det_cls[doff + d] = c;
  }
}

extern "C" int mmmot_match_dets(const double* det_xywh, const double* gt_xywh, const int* gt_id, const int* gt_name,
                                const int* frames, int NF, int car_code, int dontcare_code, double max_iou, int max_n,
                                int* det_id, int* det_cls, void* stream) {
  if (!det_xywh || !gt_xywh || !gt_id || !gt_name || !frames || !det_id || !det_cls) return MMMOT_EINVAL;
  if (NF < 1 || max_n < 1 || max_n > LB_MAXN) return MMMOT_EINVAL;
  if ((((uintptr_t)det_xywh) | ((uintptr_t)gt_xywh)) & 7u) return MMMOT_EINVAL;
  hipLaunchKernelGGL(match_dets_kernel, dim3(NF), dim3(LB_THREADS), 0, (hipStream_t)stream, det_xywh, gt_xywh, gt_id,
                     gt_name, frames, car_code, dontcare_code, max_iou, max_n, det_id, det_cls);
  return mm_check(hipGetLastError());
}
