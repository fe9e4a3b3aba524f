// HOTA and IDF1 evaluation of tracked sequences ("HOTA / IDF1"; the rules are restated in
// tests/hota_ref.py) in a fixed number of launches whatever the number of frames or sequences:
//   clear    the work tables (one memset)
//   prep     one wave per FRAME: the preparation matching (IoU gated at 0.5 - eps) and the keep flags
//   pass 1   one workgroup per SEQUENCE walks its frames IN ORDER: ID counts, pot += s / d, pm += (s >= 0.5), then align
//   pass 2   one wave per FRAME: ONE assignment maximising sum align * s, the per-alpha counts and mc
//   seq      one workgroup per SEQUENCE: frame sums in frame order, the per-alpha association sums
//   idf1     one wave per SEQUENCE: maximum-weight matching of the integer pm
//   total    one workgroup: the sums over the sequences in sequence order
// Similarities are fm_overlap's fp64 IoU (every product, sum and quotient rounded on its own).  Both per-frame
// assignments are the shortest-augmenting-path search of csrc/frame_match.h over the smaller side with cost = -value:
// every value is >= 0, so assigning all rows of the smaller side loses nothing and the pairs of value 0 are dropped
// afterwards.  Ties go to the smallest column index.
//
// Determinism: no floating-point atomics.  pot is accumulated by the one workgroup that owns the sequence, frame after
// frame with a barrier in between; within a frame a cell (gt ID, tracker ID) belongs to one thread because IDs are
// unique per frame (the host refuses tables where they are not).  LocSum is a butterfly over the wave per frame and a
// serial sum over the frames in order.  mc, pm and the counts are integers.
#include "frame_match.h"  // the box, the overlap, the limits, the frame-row check and the search

#pragma clang fp contract(off)  // every fp64 operation of this file is rounded on its own

#define HT_NA 19               // alpha_a = 0.05 (a + 1)
#define HT_MAX_CELLS (1 << 18) // G * T of one sequence
#define HT_MAX_IDS 2048        // G or T of one sequence: the potentials and labels of the IDF1 matching sit in LDS
#define HT_FRAME_D 21          // preparation assignment value, pass-2 assignment value, LocSum[19]
#define HT_FRAME_I 21          // TP[19], kept ground truth, kept tracker boxes
#define HT_SEQ_D 76            // LocSum[19], sum mc A [19], sum mc mc / gt_count [19], sum mc mc / tr_count [19]
#define HT_SEQ_I 24            // TP[19], kept ground truth, kept tracker boxes, IDTP, status, pad
#define HT_SEQ_TAB 6           // first frame, G, T, first cell, first gt ID slot, first tracker ID slot
#define HT_EPS 2.220446049250313e-16

namespace {

__device__ __forceinline__ double ht_alpha(int a) {
#pragma clang fp contract(off)
  return 0.05 * (double)(a + 1);
}

struct HtSeq {
  int f0, f1, G, T, cell0, g0, t0;
  bool ok;
};

// row s of the sequence table, checked against the sizes the launcher was given: nothing outside the work tables is
// ever addressed
__device__ __forceinline__ HtSeq ht_seq(const int* __restrict__ seq_tab, int s, int S, int NF, int cells, int sumG,
                                        int sumT) {
  HtSeq r;
  const int* q = seq_tab + HT_SEQ_TAB * s;
  r.f0 = q[0], r.G = q[1], r.T = q[2], r.cell0 = q[3], r.g0 = q[4], r.t0 = q[5];
  r.f1 = q[HT_SEQ_TAB];
  r.ok = s >= 0 && s < S && r.f0 >= 0 && r.f1 >= r.f0 && r.f1 <= NF && r.G >= 0 && r.T >= 0 && r.G <= HT_MAX_IDS &&
         r.T <= HT_MAX_IDS && (long long)r.G * r.T <= HT_MAX_CELLS && r.cell0 >= 0 && r.g0 >= 0 && r.t0 >= 0 &&
         r.cell0 <= cells - r.G * r.T && r.g0 <= sumG - r.G && r.t0 <= sumT - r.T;
  return r;
}

// what fm_assign searches for a value val(ground truth i, tracker j) >= 0: cost = -value, the rows being the smaller
// side (tr: the tracker side)
template <class V>
struct HtCost {
  const V& val;
  bool tr;
  typedef int Row;
  __device__ __forceinline__ Row row(int i) const { return i; }
  __device__ __forceinline__ double cell(int r, int c) const { return tr ? -val(c, r) : -val(r, c); }
};

template <class V>
__device__ __forceinline__ HtCost<V> ht_cost(const V& val, bool tr) {
  return HtCost<V>{val, tr};
}

// preparation: keep flags of every ground-truth and tracker row of the frame, and the value of its assignment
__global__ __launch_bounds__(64) void ht_prep_kernel(const double* __restrict__ boxes, int nG, int nT, int nD,
                                                     const int* __restrict__ frames, const int* __restrict__ g_attr,
                                                     double min_height, double max_truncation, double max_occlusion,
                                                     int prepare, int* __restrict__ gkeep, int* __restrict__ tkeep,
                                                     double* __restrict__ frame_d) {
  constexpr int K = FM_MAXN / 64;
  __shared__ FmBox gb[FM_MAXN], tb[FM_MAXN], db[FM_MAXD];
  __shared__ double u[FM_MAXN];
  __shared__ int row4col[FM_MAXN], col4row[FM_MAXN], path[FM_MAXN], mt[FM_MAXN];
  const int f = blockIdx.x, tid = threadIdx.x;
  const FmFrame fr = fm_frame(frames + 6 * f, nG, nT, nD);
  if (!fr.ok) return;  // pass 2 marks the frame; its keep flags stay 0
  const int G = fr.G, T = fr.T, D = fr.D, go = fr.go, to = fr.to;
  if (!prepare) {
    for (int i = tid; i < G; i += 64) gkeep[go + i] = g_attr[4 * (go + i) + 2] == 0 ? 1 : 0;
    for (int j = tid; j < T; j += 64) tkeep[to + j] = 1;
    if (tid == 0) frame_d[HT_FRAME_D * f] = 0.0;
    return;
  }
  const FmBox* gsrc = (const FmBox*)boxes + go;
  const FmBox* tsrc = (const FmBox*)boxes + nG + to;
  const FmBox* dsrc = (const FmBox*)boxes + nG + nT + fr.dof;
  for (int i = tid; i < G; i += 64) gb[i] = gsrc[i];
  for (int j = tid; j < T; j += 64) {
    tb[j] = tsrc[j];
    mt[j] = -1;
  }
  for (int d = tid; d < D; d += 64) db[d] = dsrc[d];
  __syncthreads();
  const bool tr = G > T;  // rows are the smaller side
  const int R = tr ? T : G, C = tr ? G : T;
  const double gate = 0.5 - HT_EPS;
  auto val = [&](int i, int j) {  // ground truth i, tracker j
    const double s = fm_overlap(gb[i], tb[j], false);
    return s < gate ? 0.0 : s;
  };
  fm_assign(R, C, tid, u, row4col, col4row, path, ht_cost(val, tr));
  double value = 0.0;
  for (int r = tid; r < R; r += 64) {
    const int c4 = col4row[r];
    if (c4 >= 0) {
      const int i = tr ? c4 : r, j = tr ? r : c4;
      const double s = val(i, j);
      if (s > HT_EPS) {
        mt[j] = i;
        value += s;
      }
    }
  }
  value = wave_sum_d(value);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int j = k * 64 + tid;
    if (j < T) {
      bool rm;
      const int i = mt[j];
      if (i >= 0) {
        const int* a = g_attr + 4 * (go + i);
        rm = a[2] == 1 || (double)a[1] > max_occlusion || (double)a[0] > max_truncation;
      } else {
#pragma clang fp contract(off)
        const FmBox b = tb[j];
        rm = b.y2 - b.y1 <= min_height + HT_EPS;
        for (int d = 0; d < D && !rm; ++d) rm = fm_overlap(b, db[d], true) > 0.5 + HT_EPS;
      }
      tkeep[to + j] = rm ? 0 : 1;
    }
    const int i = k * 64 + tid;
    if (i < G) {
      const int* a = g_attr + 4 * (go + i);
      gkeep[go + i] = (a[2] == 0 && (double)a[1] <= max_occlusion && (double)a[0] <= max_truncation) ? 1 : 0;
    }
  }
  if (tid == 0) frame_d[HT_FRAME_D * f] = value;
}

// The kept rows of one side of a frame, compacted in order into LDS by ONE wave (lane = threadIdx.x < 64): boxes and
// dense IDs.  A row whose ID lies outside [0, n_ids) is dropped.  Returns the count (the same in every lane).
__device__ __forceinline__ int ht_load_kept(const FmBox* __restrict__ src, const int* __restrict__ keep,
                                            const int* __restrict__ id, int id_stride, int n, int n_ids, int lane,
                                            FmBox* dst, int* dst_id) {
  int base = 0;
  for (int k = 0; k < FM_MAXN / 64; ++k) {
    const int i = k * 64 + lane;
    int my = -1;
    if (i < n && keep[i] != 0) my = id[id_stride * i];
    const bool kp = my >= 0 && my < n_ids;
    const unsigned long long m = __ballot(kp);
    if (kp) {
      const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
      dst[pos] = src[i];
      dst_id[pos] = my;
    }
    base += __popcll(m);
  }
  return base;
}

// pass 1: the sequence's frames in order
__global__ __launch_bounds__(256) void ht_pot_kernel(const double* __restrict__ boxes, int nG, int nT, int nD,
                                                     const int* __restrict__ frames, int NF,
                                                     const int* __restrict__ g_attr, const int* __restrict__ t_id,
                                                     const int* __restrict__ seq_tab, int S, int cells, int sumG,
                                                     int sumT, const int* __restrict__ gkeep,
                                                     const int* __restrict__ tkeep, double* pot, int* pm,
                                                     int* gcount, int* tcount) {
  __shared__ FmBox gb[FM_MAXN], tb[FM_MAXN];
  __shared__ int gid[FM_MAXN], tid_[FM_MAXN], nk[2];
  __shared__ double rs[FM_MAXN], cs[FM_MAXN];
  const int t = threadIdx.x;
  const HtSeq sq = ht_seq(seq_tab, blockIdx.x, S, NF, cells, sumG, sumT);
  if (!sq.ok) return;
  double* spot = pot + sq.cell0;
  int* spm = pm + sq.cell0;
  for (int f = sq.f0; f < sq.f1; ++f) {
    const FmFrame fr = fm_frame(frames + 6 * f, nG, nT, nD);
    if (!fr.ok) continue;  // uniform
    if (t < 64) {
      const int a = ht_load_kept((const FmBox*)boxes + fr.go, gkeep + fr.go, g_attr + 4 * fr.go + 3, 4, fr.G, sq.G, t,
                                 gb, gid);
      const int b = ht_load_kept((const FmBox*)boxes + nG + fr.to, tkeep + fr.to, t_id + fr.to, 1, fr.T, sq.T, t, tb,
                                 tid_);
      if (t == 0) {
        nk[0] = a;
        nk[1] = b;
      }
    }
    __syncthreads();
    const int Gk = nk[0], Tk = nk[1];
    if (t < FM_MAXN) {
      if (t < Gk) {
        gcount[sq.g0 + gid[t]] += 1;
        double a = 0.0;
        for (int j = 0; j < Tk; ++j) a += fm_overlap(gb[t], tb[j], false);
        rs[t] = a;
      }
    } else if (t - FM_MAXN < Tk) {
      const int j = t - FM_MAXN;
      tcount[sq.t0 + tid_[j]] += 1;
      double a = 0.0;
      for (int i = 0; i < Gk; ++i) a += fm_overlap(gb[i], tb[j], false);
      cs[j] = a;
    }
    __syncthreads();
    for (int p = t; p < Gk * Tk; p += 256) {
#pragma clang fp contract(off)
      const int i = p / Tk, j = p - i * Tk;
      const double s = fm_overlap(gb[i], tb[j], false);
      if (s > 0.0) {
        const int c = gid[i] * sq.T + tid_[j];
        const double d = cs[j] + rs[i] - s;
        if (d > HT_EPS) spot[c] += s / d;
        if (s >= 0.5) spm[c] += 1;
      }
    }
    __syncthreads();
  }
  __syncthreads();
  // align = pot / (gt_count + tr_count - pot), in place
  for (int c = t; c < sq.G * sq.T; c += 256) {
#pragma clang fp contract(off)
    const int i = c / sq.T, j = c - i * sq.T;
    const double p = spot[c];
    const double d = (double)(gcount[sq.g0 + i] + tcount[sq.t0 + j]) - p;
    spot[c] = d > 0.0 ? p / d : 0.0;
  }
}

// pass 2: one assignment per frame, counted at every alpha
__global__ __launch_bounds__(64) void ht_match_kernel(const double* __restrict__ boxes, int nG, int nT, int nD,
                                                      const int* __restrict__ frames, int NF,
                                                      const int* __restrict__ frame_seq,
                                                      const int* __restrict__ g_attr, const int* __restrict__ t_id,
                                                      const int* __restrict__ seq_tab, int S, int cells, int sumG,
                                                      int sumT, const int* __restrict__ gkeep,
                                                      const int* __restrict__ tkeep, const double* __restrict__ align,
                                                      int* __restrict__ mc, double* __restrict__ frame_d,
                                                      int* __restrict__ frame_i) {
  constexpr int K = FM_MAXN / 64;
  __shared__ FmBox gb[FM_MAXN], tb[FM_MAXN];
  __shared__ int gid[FM_MAXN], tid_[FM_MAXN];
  __shared__ double u[FM_MAXN];
  __shared__ int row4col[FM_MAXN], col4row[FM_MAXN], path[FM_MAXN];
  const int f = blockIdx.x, tid = threadIdx.x;
  double* fd = frame_d + HT_FRAME_D * f;
  int* fi = frame_i + HT_FRAME_I * f;
  const FmFrame fr = fm_frame(frames + 6 * f, nG, nT, nD);
  const int s = frame_seq[f];
  HtSeq sq;
  sq.ok = false;
  if (s >= 0 && s < S) sq = ht_seq(seq_tab, s, S, NF, cells, sumG, sumT);
  if (!fr.ok || !sq.ok || f < sq.f0 || f >= sq.f1) {  // outside the contract: a marked frame, nothing is read
    if (tid < HT_FRAME_I) fi[tid] = -1;
    if (tid < HT_FRAME_D) fd[tid] = __builtin_nan("");
    return;
  }
  const int G = ht_load_kept((const FmBox*)boxes + fr.go, gkeep + fr.go, g_attr + 4 * fr.go + 3, 4, fr.G, sq.G, tid, gb,
                             gid);
  const int T = ht_load_kept((const FmBox*)boxes + nG + fr.to, tkeep + fr.to, t_id + fr.to, 1, fr.T, sq.T, tid, tb,
                             tid_);
  __syncthreads();
  const double* al = align + sq.cell0;
  const bool tr = G > T;
  const int R = tr ? T : G, C = tr ? G : T;
  auto val = [&](int i, int j) {
#pragma clang fp contract(off)
    return al[gid[i] * sq.T + tid_[j]] * fm_overlap(gb[i], tb[j], false);
  };
  fm_assign(R, C, tid, u, row4col, col4row, path, ht_cost(val, tr));
  double sv[K], value = 0.0;
  int cell[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int r = k * 64 + tid;
    sv[k] = -1.0;
    cell[k] = 0;
    if (r < R && col4row[r] >= 0) {
      const int c4 = col4row[r];
      const int i = tr ? c4 : r, j = tr ? r : c4;
      sv[k] = fm_overlap(gb[i], tb[j], false);
      cell[k] = gid[i] * sq.T + tid_[j];
      value += val(i, j);
    }
  }
  value = wave_sum_d(value);
  int* smc = mc + (long long)HT_NA * sq.cell0;
  const int GT = sq.G * sq.T;
  for (int a = 0; a < HT_NA; ++a) {
#pragma clang fp contract(off)
    const double thr = ht_alpha(a) - HT_EPS;
    int n = 0;
    double loc = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const bool hit = sv[k] >= thr;
      n += fm_count(hit);
      if (hit) {
        loc += sv[k];
        atomicAdd(smc + (long long)a * GT + cell[k], 1);
      }
    }
    loc = wave_sum_d(loc);
    if (tid == 0) {
      fi[a] = n;
      fd[2 + a] = loc;
    }
  }
  if (tid == 0) {
    fi[HT_NA] = G;
    fi[HT_NA + 1] = T;
    fd[1] = value;
  }
}

// per sequence: the frame sums in frame order and the association sums of every alpha
__global__ __launch_bounds__(256) void ht_seq_kernel(const int* __restrict__ seq_tab, int S, int NF, int cells, int sumG,
                                                     int sumT, const double* __restrict__ frame_d,
                                                     const int* __restrict__ frame_i, const int* __restrict__ mc,
                                                     const int* __restrict__ gcount, const int* __restrict__ tcount,
                                                     double* __restrict__ seq_d, int* __restrict__ seq_i) {
  __shared__ double red[3][4];
  const int s = blockIdx.x, t = threadIdx.x;
  double* sd = seq_d + HT_SEQ_D * s;
  int* si = seq_i + HT_SEQ_I * s;
  const HtSeq sq = ht_seq(seq_tab, s, S, NF, cells, sumG, sumT);
  if (!sq.ok) {
    if (t < HT_SEQ_I) si[t] = -1;
    if (t < HT_SEQ_D) sd[t] = __builtin_nan("");
    return;
  }
  if (t < HT_FRAME_I) {  // TP[19], kept ground truth, kept tracker boxes
    int a = 0, bad = 0;
    for (int f = sq.f0; f < sq.f1; ++f) {
      const int v = frame_i[HT_FRAME_I * f + t];
      bad |= v < 0 ? 1 : 0;
      a += v;
    }
    si[t] = bad ? -1 : a;
    if (t == 0) {
      si[HT_NA + 3] = bad ? -1 : 0;
      si[HT_NA + 4] = 0;
    }
  } else if (t >= 64 && t < 64 + HT_NA) {  // LocSum
    double a = 0.0;
    for (int f = sq.f0; f < sq.f1; ++f) a += frame_d[HT_FRAME_D * f + 2 + (t - 64)];
    sd[t - 64] = a;
  }
  const int GT = sq.G * sq.T;
  const int* smc = mc + (long long)HT_NA * sq.cell0;
  for (int a = 0; a < HT_NA; ++a) {
    double sA = 0.0, sR = 0.0, sP = 0.0;
    for (int c = t; c < GT; c += 256) {
#pragma clang fp contract(off)
      const int m = smc[(long long)a * GT + c];
      if (m != 0) {
        const int i = c / sq.T, j = c - i * sq.T;
        const int gc = gcount[sq.g0 + i], tc = tcount[sq.t0 + j];
        const int den = gc + tc - m;
        const double dm = (double)m;
        sA += dm * (dm / (double)(den > 1 ? den : 1));
        sR += dm * (dm / (double)(gc > 1 ? gc : 1));
        sP += dm * (dm / (double)(tc > 1 ? tc : 1));
      }
    }
    sA = wave_sum_d(sA);
    sR = wave_sum_d(sR);
    sP = wave_sum_d(sP);
    __syncthreads();
    if ((t & 63) == 0) {
      red[0][t >> 6] = sA;
      red[1][t >> 6] = sR;
      red[2][t >> 6] = sP;
    }
    __syncthreads();
    if (t < 3) sd[HT_NA * (1 + t) + a] = ((red[t][0] + red[t][1]) + red[t][2]) + red[t][3];
  }
}

// IDF1: the G x T maximum-weight matching of the integer pm with unmatched rows and columns free, which is the
// assignment of every row of the smaller side at cost -pm (every weight is >= 0).  Integer potentials in LDS, the
// cost rows in global memory, lanes over the columns, ties to the smallest column.
__global__ __launch_bounds__(64) void ht_idf1_kernel(const int* __restrict__ seq_tab, int S, int NF, int cells, int sumG,
                                                     int sumT, const int* __restrict__ pm, int* __restrict__ seq_i) {
  __shared__ int u[HT_MAX_IDS], col4row[HT_MAX_IDS];
  __shared__ int v[HT_MAX_IDS], sp[HT_MAX_IDS], path[HT_MAX_IDS], row4col[HT_MAX_IDS];
  __shared__ unsigned char scanned[HT_MAX_IDS];
  const int s = blockIdx.x, lane = threadIdx.x;
  const HtSeq sq = ht_seq(seq_tab, s, S, NF, cells, sumG, sumT);
  if (!sq.ok) return;  // the sequence kernel marked the row
  const int* w = pm + sq.cell0;
  const bool tr = sq.G > sq.T;
  const int R = tr ? sq.T : sq.G, C = tr ? sq.G : sq.T;
  auto weight = [&](int r, int c) { return tr ? w[c * sq.T + r] : w[r * sq.T + c]; };
  for (int r = lane; r < R; r += 64) {
    u[r] = 0;
    col4row[r] = -1;
  }
  for (int j = lane; j < C; j += 64) {
    v[j] = 0;
    row4col[j] = -1;
    path[j] = -1;
  }
  __syncthreads();
  for (int cur = 0; cur < R; ++cur) {
    for (int j = lane; j < C; j += 64) {
      sp[j] = 0x7fffffff;
      scanned[j] = 0;
    }
    __syncthreads();
    int minv = 0, i = cur, sink = -1;
    for (;;) {
      const int ui = u[i];
      int bv = 0x7fffffff, bj = 0x7fffffff;
      for (int j = lane; j < C; j += 64) {
        if (!scanned[j]) {
          const int r = minv - weight(i, j) - ui - v[j];
          if (r < sp[j]) {
            sp[j] = r;
            path[j] = i;
          }
          if (sp[j] < bv) {  // ascending j: the first smallest stays
            bv = sp[j];
            bj = j;
          }
        }
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const int ov = __shfl_xor(bv, o), oj = __shfl_xor(bj, o);
        if (ov < bv || (ov == bv && oj < bj)) {
          bv = ov;
          bj = oj;
        }
      }
      if (bj >= C) break;  // cannot happen: C >= R
      minv = bv;
      if (lane == 0) scanned[bj] = 1;
      __syncthreads();
      const int nxt = row4col[bj];
      if (nxt < 0) {
        sink = bj;
        break;
      }
      i = nxt;
    }
    if (sink >= 0) {
      for (int j = lane; j < C; j += 64) {
        if (scanned[j]) {
          const int d = minv - sp[j];
          v[j] -= d;
          if (j != sink) u[row4col[j]] += d;
        }
      }
      if (lane == 0) u[cur] += minv;
    }
    __syncthreads();
    if (lane == 0 && sink >= 0) {
      int j = sink;
      for (;;) {
        const int r = path[j];
        row4col[j] = r;
        const int prev = col4row[r];
        col4row[r] = j;
        j = prev;
        if (r == cur) break;
      }
    }
    __syncthreads();
  }
  int m = 0;
  for (int r = lane; r < R; r += 64)
    if (col4row[r] >= 0) m += weight(r, col4row[r]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m += __shfl_xor(m, o);
  if (lane == 0) seq_i[HT_SEQ_I * s + HT_NA + 2] = m;
}

// totals into row S, the sequences in order: the integers and LocSum add; the association sums become the TP-weighted
// sums  sum_s (num_s / max(1, TP_s)) * TP_s  of step 4
__global__ __launch_bounds__(128) void ht_total_kernel(int S, double* __restrict__ seq_d, int* __restrict__ seq_i) {
  const int t = threadIdx.x;
  if (t < HT_SEQ_I) {
    int a = 0, bad = 0;
    for (int s = 0; s < S; ++s) {
      a += seq_i[HT_SEQ_I * s + t];
      bad |= seq_i[HT_SEQ_I * s + HT_NA + 3] < 0 ? 1 : 0;
    }
    seq_i[HT_SEQ_I * S + t] = t == HT_NA + 3 ? (bad ? -1 : 0) : a;
  } else if (t >= 32 && t < 32 + HT_SEQ_D) {
#pragma clang fp contract(off)
    const int q = t - 32, al = q % HT_NA;
    double a = 0.0;
    for (int s = 0; s < S; ++s) {
      const double x = seq_d[HT_SEQ_D * s + q];
      if (q < HT_NA) {
        a += x;
      } else {
        const int tp = seq_i[HT_SEQ_I * s + al];
        a += (x / (double)(tp > 1 ? tp : 1)) * (double)tp;
      }
    }
    seq_d[HT_SEQ_D * S + q] = a;
  }
}

}  // namespace

extern "C" int mmmot_hota(const double* boxes, int nG, int nT, int nD, const int* frames, int NF, const int* frame_seq,
                          const int* g_attr, const int* t_id, const int* seq_tab, int S, int cells, int sumG, int sumT,
                          int max_boxes, int max_dontcare, double min_height, double max_truncation,
                          double max_occlusion, int prepare, void* work, long long work_bytes, double* frame_d,
                          int* frame_i, double* seq_d, int* seq_i, void* stream) {
  if (nG < 0 || nT < 0 || nD < 0 || NF < 0 || S < 1 || cells < 0 || sumG < 0 || sumT < 0) return MMMOT_EINVAL;
  if (max_boxes < 0 || max_boxes > FM_MAXN || max_dontcare < 0 || max_dontcare > FM_MAXD) return MMMOT_EINVAL;
  if ((long long)cells > (long long)S * HT_MAX_CELLS || (long long)sumG > (long long)S * HT_MAX_IDS ||
      (long long)sumT > (long long)S * HT_MAX_IDS)
    return MMMOT_EINVAL;
  if (prepare != 0 && prepare != 1) return MMMOT_EINVAL;
  if (!seq_tab || !seq_d || !seq_i || !work) return MMMOT_EINVAL;
  if (NF > 0 && (!frames || !frame_seq || !frame_d || !frame_i)) return MMMOT_EINVAL;
  if (nG + nT + nD > 0 && !boxes) return MMMOT_EINVAL;
  if (nG > 0 && !g_attr) return MMMOT_EINVAL;
  if (nT > 0 && !t_id) return MMMOT_EINVAL;
  if ((((uintptr_t)boxes) | ((uintptr_t)frame_d) | ((uintptr_t)seq_d) | ((uintptr_t)work)) & 7u) return MMMOT_EINVAL;
  // work: pot fp64 [cells] | mc int32 [19 cells] | pm [cells] | gt_count [sumG] | tr_count [sumT] | gkeep [nG] | tkeep [nT]
  const long long need = 8LL * cells + 4LL * ((long long)HT_NA * cells + cells + sumG + sumT + nG + nT);
  if (work_bytes < need) return MMMOT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  double* pot = (double*)work;
  int* mc = (int*)(pot + cells);
  int* pm = mc + (long long)HT_NA * cells;
  int* gcount = pm + cells;
  int* tcount = gcount + sumG;
  int* gkeep = tcount + sumT;
  int* tkeep = gkeep + nG;
  if (need > 0) {
    const hipError_t e = hipMemsetAsync(work, 0, (size_t)need, st);
    if (e != hipSuccess) return mm_check(e);
  }
  if (NF > 0)
    hipLaunchKernelGGL(ht_prep_kernel, dim3(NF), dim3(64), 0, st, boxes, nG, nT, nD, frames, g_attr, min_height,
                       max_truncation, max_occlusion, prepare, gkeep, tkeep, frame_d);
  hipLaunchKernelGGL(ht_pot_kernel, dim3(S), dim3(256), 0, st, boxes, nG, nT, nD, frames, NF, g_attr, t_id, seq_tab, S,
                     cells, sumG, sumT, gkeep, tkeep, pot, pm, gcount, tcount);
  if (NF > 0)
    hipLaunchKernelGGL(ht_match_kernel, dim3(NF), dim3(64), 0, st, boxes, nG, nT, nD, frames, NF, frame_seq, g_attr,
                       t_id, seq_tab, S, cells, sumG, sumT, gkeep, tkeep, pot, mc, frame_d, frame_i);
  hipLaunchKernelGGL(ht_seq_kernel, dim3(S), dim3(256), 0, st, seq_tab, S, NF, cells, sumG, sumT, frame_d, frame_i, mc,
                     gcount, tcount, seq_d, seq_i);
  hipLaunchKernelGGL(ht_idf1_kernel, dim3(S), dim3(64), 0, st, seq_tab, S, NF, cells, sumG, sumT, pm, seq_i);
  hipLaunchKernelGGL(ht_total_kernel, dim3(1), dim3(128), 0, st, S, seq_d, seq_i);
  return mm_check(hipGetLastError());
}
