// Smoothing of tracked sequences: a Kalman filter forwards and a Rauch-Tung-Striebel pass backwards along every track
// (see include/mmmot_hip.h: mmmot_smooth_tracks; DESIGN section 12b, whose operation order this file follows).
//
// Five launches whatever the number of rows, frames, sequences or tracks:
//   st_check  one thread per table entry: ft_check_entry of track_links.h
//   st_link   one thread per detection: its frame, duplicates, its successor; the predecessor is the successor
//             scattered back
//   st_heads  one thread per detection: the first observed row of a track that has a successor heads a chain; the heads
//             are compacted by an integer atomic (the order of the list varies, no output word depends on it)
//   st_chain  8 lanes per head: x, y, z, yaw, h, w, l and a marker; a lane walks the chain forwards, keeps the filtered
//             values in the scratch, and walks back
//   st_store  one thread per row: copy, and for marked rows the back transform, the wrap, the rounding, the stores
// Integer atomics only; every output word has one writer, so two calls give the same bits.  fp64 with every product,
// sum and quotient rounded on its own (`#pragma clang fp contract(off)`), one rounding to fp32 at the store.
#include "common.h"
#include "track_links.h"

#define ST_THREADS 256
#define ST_VALS 5                   // doubles per row and channel: p, v, P00, P01, P11 (h w l: p, P)
#define ST_CH 7                     // x, y, z, yaw, h, w, l
#define ST_ROW (ST_VALS * ST_CH)    // doubles per row
#define ST_PI 3.141592653589793
#define ST_TWO_PI 6.283185307179586
#define ST_HALF_PI 1.5707963267948966
#define ST_WRAP_STEPS 4096

struct st_params {
  double q[3], r[3], v0[3];  // groups: 0 location, 1 yaw, 2 h w l (v0[2] unused)
  int yaw_flip;
};

// the int tables behind the 35 L doubles of the scratch
struct st_work {
  double* val;
  int *flag, *count, *mark, *pred, *frame, *succ, *heads;
};

__host__ __device__ __forceinline__ st_work st_split(int* work, long L) {
  st_work w;
  w.val = (double*)work;
  int* t = work + 2 * ST_ROW * L;
  w.flag = t, w.count = t + 1, w.mark = t + 2;
  w.pred = w.mark + L, w.frame = w.pred + L, w.succ = w.frame + L, w.heads = w.succ + L;
  return w;
}

__global__ __launch_bounds__(ST_THREADS) void st_check_kernel(const int* __restrict__ frame_start,
                                                              const int* __restrict__ frame_no,
                                                              const int* __restrict__ seq_start, int L, int F, int S,
                                                              int* __restrict__ work, int* __restrict__ info) {
  ft_check_entry(blockIdx.x * ST_THREADS + threadIdx.x, frame_start, frame_no, seq_start, L, F, S,
                 st_split(work, L).flag, info);
}

__global__ __launch_bounds__(ST_THREADS) void st_link_kernel(const int* __restrict__ ids,
                                                             const int* __restrict__ frame_start,
                                                             const int* __restrict__ seq_start, int L, int F, int S,
                                                             int* __restrict__ work, int* __restrict__ info) {
  const int i = blockIdx.x * ST_THREADS + threadIdx.x;
  const st_work w = st_split(work, L);
  if (i >= L || *w.flag) return;
  const int pa = ft_last_le(frame_start, F, i);
  const int s = ft_last_le(seq_start, S, pa);
  const int id = ids[i];
  int sj = -1;
  if (id >= 0) {
    if (ft_dup_in_frame(ids, frame_start, pa, i, id)) atomicOr(&info[4 * s], MMMOT_FILL_EDUP);
    int pb;
    sj = ft_successor(ids, frame_start, pa, seq_start[s + 1], id, pb);
    if (sj >= 0) w.pred[sj] = i;  // sj in (i, L): found through a checked frame_start
  }
  w.frame[i] = pa;
  w.succ[i] = sj;
}

__global__ __launch_bounds__(ST_THREADS) void st_heads_kernel(const int* __restrict__ ids,
                                                              const int* __restrict__ seq_start,
                                                              const int* __restrict__ observed, int L, int S,
                                                              int any, int* __restrict__ work,
                                                              int* __restrict__ info) {
  const int i = blockIdx.x * ST_THREADS + threadIdx.x;
  const st_work w = st_split(work, L);
  if (i >= L || !any || *w.flag) return;  // with every r = 0 no chain is smoothed: the head list stays empty
  if (ids[i] < 0 || w.succ[i] < 0 || (observed && !observed[i])) return;
  const int s = ft_last_le(seq_start, S, w.frame[i]);
  if (info[4 * s] != 0) return;  // only status bits are set before this launch
  if (observed) {
    for (int c = w.pred[i]; c >= 0; c = w.pred[c])  // pred strictly decreases: the walk ends
      if (observed[c]) return;
  } else if (w.pred[i] >= 0) {
    return;
  }
  w.heads[atomicAdd(w.count, 1)] = i;  // at most one head per track, each with a successor: fewer than L
  atomicAdd(&info[4 * s + 1], 1);
}

// the prediction of one constant-velocity step of d frame numbers from the filtered (p, v, P00, P01, P11)
struct st_pred {
  double pp, vp, A, B, C, t1, t2;
};

__device__ __forceinline__ st_pred st_predict(double p, double v, double P00, double P01, double P11, double d,
                                              double q) {
#pragma clang fp contract(off)
  st_pred o;
  const double d2 = d * d;
  const double d3 = d2 * d;
  const double q00 = q * (d3 / 3.0);
  const double q01 = q * (d2 / 2.0);
  const double q11 = q * d;
  o.t1 = d * P01;
  o.t2 = d * P11;
  o.pp = p + d * v;
  o.vp = v;
  double a = P00 + o.t1;
  a = a + o.t1;
  a = a + d * o.t2;
  o.A = a + q00;
  o.B = (P01 + o.t2) + q01;
  o.C = P11 + q11;
  return o;
}

// into [-pi, pi) by at most four steps of 2 pi (ft_wrap of fill_tracks.hip)
__device__ __forceinline__ double st_wrap4(double d) {
#pragma clang fp contract(off)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (d >= ST_PI) d = d - ST_TWO_PI;
    else if (d < -ST_PI) d = d + ST_TWO_PI;
  }
  return d;
}

__global__ __launch_bounds__(ST_THREADS) void st_chain_kernel(const float* __restrict__ det,
                                                              const int* __restrict__ frame_no,
                                                              const int* __restrict__ observed,
                                                              const double* __restrict__ xf0, int L, st_params prm,
                                                              int* __restrict__ work) {
#pragma clang fp contract(off)
  const long lane = (long)blockIdx.x * ST_THREADS + threadIdx.x;
  const st_work w = st_split(work, L);
  if (*w.flag) return;
  const int h = (int)(lane >> 3), ch = (int)(lane & 7);
  if (h >= *w.count) return;
  const int head = w.heads[h];
  if (ch == 7) {
    for (int i = head; i >= 0; i = w.succ[i]) w.mark[i] = 1;
    return;
  }
  const int grp = ch < 3 ? 0 : (ch == 3 ? 1 : 2);
  const double q = prm.q[grp], r = prm.r[grp];
  if (!(r > 0.0)) return;
  double p = 0.0, v = 0.0, P00 = r, P01 = 0.0, P11 = prm.v0[grp];
  double yprev = 0.0, u = 0.0;
  int last = head, prev_no = 0;
  for (int i = head; i >= 0; i = w.succ[i]) {
    const int fr = w.frame[i];
    const bool obs = !observed || observed[i] != 0;
    double z = 0.0;
    if (obs) {
      const float* __restrict__ a = det + (long)i * 12;
      const double* __restrict__ rec = xf0 ? xf0 + (long)fr * MMMOT_FILL_REC : nullptr;
      if (ch < 3) {
        if (rec) {
          const double x = (double)a[7], y = (double)a[8], zz = (double)a[9];
          double s = x * rec[0 + ch] + y * rec[4 + ch];
          s = s + zz * rec[8 + ch];
          z = s + rec[12 + ch];
        } else {
          z = (double)a[7 + ch];
        }
      } else if (ch == 3) {
        double y = (double)a[10];
        if (rec) y = y + rec[32];
        if (i == head) {
          u = y;
        } else {
          double e = st_wrap4(y - yprev);
          if (prm.yaw_flip && (e > ST_HALF_PI || e < -ST_HALF_PI)) e = st_wrap4(e + ST_PI);
          u = u + e;
        }
        yprev = y;
        z = u;
      } else {
        z = (double)a[ch];  // h w l at 4..6
      }
    }
    const int no = frame_no[fr];
    if (i == head) {
      p = z;  // the head is observed
    } else {
      const double d = (double)((long long)no - (long long)prev_no);
      if (ch < 4) {
        const st_pred o = st_predict(p, v, P00, P01, P11, d, q);
        if (obs) {
          const double s = o.A + r;
          const double k0 = o.A / s, k1 = o.B / s;
          const double e = z - o.pp;
          p = o.pp + k0 * e;
          v = o.vp + k1 * e;
          P00 = o.A - k0 * o.A;
          P01 = o.B - k0 * o.B;
          P11 = o.C - k1 * o.B;
        } else {
          p = o.pp, v = o.vp, P00 = o.A, P01 = o.B, P11 = o.C;
        }
      } else {
        const double A = P00 + q * d;
        if (obs) {
          const double s = A + r;
          const double k0 = A / s;
          p = p + k0 * (z - p);
          P00 = A - k0 * A;
        } else {
          P00 = A;
        }
      }
    }
    double* __restrict__ o = w.val + ((long)i * ST_CH + ch) * ST_VALS;
    o[0] = p;
    if (ch < 4) {
      o[1] = v, o[2] = P00, o[3] = P01, o[4] = P11;
    } else {
      o[1] = P00;
    }
    prev_no = no;
    last = i;
  }
  // backwards: the last row's smoothed values are its filtered ones, already in place
  double ps = p, vs = v;
  int next_no = prev_no;
  for (int i = last == head ? -1 : w.pred[last]; i >= 0; i = i == head ? -1 : w.pred[i]) {
    double* __restrict__ o = w.val + ((long)i * ST_CH + ch) * ST_VALS;
    const int no = frame_no[w.frame[i]];
    const double d = (double)((long long)next_no - (long long)no);
    if (ch < 4) {
      const double fp = o[0], fv = o[1], f00 = o[2], f01 = o[3], f11 = o[4];
      const st_pred n = st_predict(fp, fv, f00, f01, f11, d, q);
      const double c00 = f00 + n.t1, c10 = f01 + n.t2;
      const double dt = n.A * n.C - n.B * n.B;
      const double g00 = (c00 * n.C - f01 * n.B) / dt;
      const double g01 = (f01 * n.A - c00 * n.B) / dt;
      const double g10 = (c10 * n.C - f11 * n.B) / dt;
      const double g11 = (f11 * n.A - c10 * n.B) / dt;
      const double ep = ps - n.pp, ev = vs - n.vp;
      ps = fp + (g00 * ep + g01 * ev);
      vs = fv + (g10 * ep + g11 * ev);
      o[0] = ps, o[1] = vs;
    } else {
      const double fp = o[0], fP = o[1];
      const double A = fP + q * d;
      const double g = fP / A;
      ps = fp + g * (ps - fp);
      o[0] = ps;
    }
    next_no = no;
  }
}

__global__ __launch_bounds__(ST_THREADS) void st_store_kernel(const float* __restrict__ det,
                                                              const int* __restrict__ seq_start,
                                                              const double* __restrict__ xf0, int L, int S,
                                                              st_params prm, int* __restrict__ work,
                                                              float* __restrict__ out, float* __restrict__ out_vel,
                                                              int* __restrict__ info) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * ST_THREADS + threadIdx.x;
  const st_work w = st_split(work, L);
  const bool bad = *w.flag != 0;
  if (bad && i < S) info[4 * i] = MMMOT_FILL_ECONTRACT, info[4 * i + 1] = info[4 * i + 2] = info[4 * i + 3] = 0;
  if (i >= L) return;
  const unsigned* __restrict__ src = (const unsigned*)det + (long)i * 12;
  unsigned* __restrict__ dst = (unsigned*)out + (long)i * 12;
  const bool marked = !bad && w.mark[i] != 0;
#pragma unroll
  for (int k = 0; k < 12; ++k)
    if (!marked || k < 4 || k == 11 || !(prm.r[k < 7 ? 2 : (k < 10 ? 0 : 1)] > 0.0)) dst[k] = src[k];
  float vel[4] = {0.f, 0.f, 0.f, 0.f};
  if (!bad) {
    const int fr = w.frame[i];
    const int s = ft_last_le(seq_start, S, fr);
    atomicAdd(&info[4 * s + (marked ? 2 : 3)], 1);
    if (marked) {
      const double* __restrict__ val = w.val + (long)i * ST_ROW;
      const double* __restrict__ rec = xf0 ? xf0 + (long)fr * MMMOT_FILL_REC : nullptr;
      float* __restrict__ o = out + (long)i * 12;
      if (prm.r[0] > 0.0) {
        double x = val[0 * ST_VALS], y = val[1 * ST_VALS], z = val[2 * ST_VALS];
        double vx = val[0 * ST_VALS + 1], vy = val[1 * ST_VALS + 1], vz = val[2 * ST_VALS + 1];
        if (rec) {
          const double* __restrict__ M = rec + 16;
          double pr[3], vr[3];
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            double t = x * M[0 + j] + y * M[4 + j];
            t = t + z * M[8 + j];
            pr[j] = t + M[12 + j];
            double u = vx * M[0 + j] + vy * M[4 + j];
            vr[j] = u + vz * M[8 + j];
          }
          x = pr[0], y = pr[1], z = pr[2];
          vx = vr[0], vy = vr[1], vz = vr[2];
        }
        o[7] = (float)x, o[8] = (float)y, o[9] = (float)z;
        vel[0] = (float)vx, vel[1] = (float)vy, vel[2] = (float)vz;
      }
      if (prm.r[1] > 0.0) {
        double y = val[3 * ST_VALS];
        if (rec) y = y - rec[32];
        for (int k = 0; k < ST_WRAP_STEPS && y >= ST_PI; ++k) y = y - ST_TWO_PI;
        for (int k = 0; k < ST_WRAP_STEPS && y < -ST_PI; ++k) y = y + ST_TWO_PI;
        o[10] = (float)y;
        vel[3] = (float)val[3 * ST_VALS + 1];
      }
      if (prm.r[2] > 0.0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[4 + c] = (float)val[(4 + c) * ST_VALS];
      }
    }
  }
  if (out_vel) {
#pragma unroll
    for (int k = 0; k < 4; ++k) out_vel[(long)i * 4 + k] = vel[k];
  }
}

static bool st_param_ok(double v) { return v >= 0.0 && v <= 1.79769313486231570815e308; }  // no NaN, no infinity

extern "C" int mmmot_smooth_tracks(const float* det, const int* ids, const int* frame_start, const int* frame_no,
                                   const int* seq_start, const int* observed, const double* xf0, int L, int F, int S,
                                   double q_loc, double r_loc, double v0_loc, double q_yaw, double r_yaw, double v0_yaw,
                                   double q_dim, double r_dim, int yaw_flip, int* work, float* out, float* out_vel,
                                   int* info, void* hip_stream) {
  if (S < 1 || L < 0 || F < 0 || (yaw_flip != 0 && yaw_flip != 1)) return MMMOT_EINVAL;
  const double prm_in[8] = {q_loc, r_loc, v0_loc, q_yaw, r_yaw, v0_yaw, q_dim, r_dim};
  for (double v : prm_in)
    if (!st_param_ok(v)) return MMMOT_EINVAL;
  if ((r_loc > 0.0 && !(v0_loc > 0.0)) || (r_yaw > 0.0 && !(v0_yaw > 0.0))) return MMMOT_EINVAL;
  if (L == 0 || F == 0) return MMMOT_OK;
  if (!det || !ids || !frame_start || !frame_no || !seq_start || !work || !out || !info) return MMMOT_EINVAL;
  if (((size_t)work & 7) != 0 || MMMOT_SMOOTH_WORK(L) > 0x7fffffffL) return MMMOT_EINVAL;
  st_params prm;
  prm.q[0] = q_loc, prm.r[0] = r_loc, prm.v0[0] = v0_loc;
  prm.q[1] = q_yaw, prm.r[1] = r_yaw, prm.v0[1] = v0_yaw;
  prm.q[2] = q_dim, prm.r[2] = r_dim, prm.v0[2] = 0.0;
  prm.yaw_flip = yaw_flip;
  const bool any = r_loc > 0.0 || r_yaw > 0.0 || r_dim > 0.0;
  hipStream_t st = (hipStream_t)hip_stream;
  const st_work w = st_split(work, L);
  int rc = mm_check(hipMemsetAsync(w.flag, 0, sizeof(int) * (2 + (size_t)L), st));  // flag, count, mark
  if (rc != MMMOT_OK) return rc;
  rc = mm_check(hipMemsetAsync(w.pred, 0xff, sizeof(int) * (size_t)L, st));
  if (rc != MMMOT_OK) return rc;
  rc = mm_check(hipMemsetAsync(info, 0, sizeof(int) * 4 * (size_t)S, st));
  if (rc != MMMOT_OK) return rc;
  const int n_tab = F > S ? F : S, n_row = L > S ? L : S;
  const auto blocks = [](long n) { return dim3((unsigned)(n > ST_THREADS ? (n + ST_THREADS - 1) / ST_THREADS : 1)); };
  hipLaunchKernelGGL(st_check_kernel, blocks(n_tab), dim3(ST_THREADS), 0, st, frame_start, frame_no, seq_start, L, F, S,
                     work, info);
  hipLaunchKernelGGL(st_link_kernel, blocks(L), dim3(ST_THREADS), 0, st, ids, frame_start, seq_start, L, F, S, work,
                     info);
  hipLaunchKernelGGL(st_heads_kernel, blocks(L), dim3(ST_THREADS), 0, st, ids, seq_start, observed, L, S, (int)any,
                     work, info);
  hipLaunchKernelGGL(st_chain_kernel, blocks(8 * (long)(L / 2)), dim3(ST_THREADS), 0, st, det, frame_no, observed, xf0,
                     L, prm, work);
  hipLaunchKernelGGL(st_store_kernel, blocks(n_row), dim3(ST_THREADS), 0, st, det, seq_start, xf0, L, S, prm, work, out,
                     out_vel, info);
  return mm_check(hipGetLastError());
}
