// The CLEAR-MOT frame evaluation, once, for both cost sources: the association (the search of csrc/frame_match.h over the
// gated cost), the gate, the ignore logic and the counters of csrc/clear_mot.hip, parametrised by a cost functor - the 2D
// boxes in LDS (clear_mot.hip) or a per-frame table of c (mot3d.hip) - and the trajectory / sequence / total kernels with
// a level dimension (blockIdx.y; the 2D evaluator launches one level).  Included by one .hip file each; everything is
// file-local.
//
// A cost functor F provides
//   void bind(gb, tb)           receives the frame's 2D boxes in LDS (ground truth, tracker columns)
//   F::Row                      what the search keeps of its current row
//   Row row(bool tr, int i)     the row handle of row i (tr: the rows are the tracker side)
//   double cell(row, tr, j)     c of (row, column j)
//   double c(int i, int j)      c of ground truth i and tracker column j
//   int col(int j)              the frame's tracker object behind column j (the sweep keeps a subset of the columns)
//   void matched(i, j, tp)      called once per ground-truth object: its column or -1, and whether it counts as a true
//                               positive that is not ignored
// and the arithmetic never depends on F beyond the value of c.
#pragma once
#include "frame_match.h"  // the box, the overlap, the limits, the frame-row check and the search

#define CM_K 128.0
#define CM_SEQ_INTS 12  // tp, itp, fn, ifn, fp, n_itr, id switches, fragments, MT, PT, ML, ignored trajectories

namespace {

// c = 1 - IoU of ground truth g and tracker t
__device__ __forceinline__ double cm_c(const FmBox& g, const FmBox& t) {
#pragma clang fp contract(off)
  return 1.0 - fm_overlap(g, t, false);
}

__device__ __forceinline__ double cm_cost(double c, double min_overlap) { return c <= min_overlap ? c - CM_K : 0.0; }

// a frame outside the contract: a marked frame, nothing is read
__device__ __forceinline__ void cm_frame_mark(double* fd, int* fi) {
  const int tid = threadIdx.x;
  if (tid < 6) fi[tid] = -1;
  if (tid < 2) fd[tid] = __builtin_nan("");
}

// the cost from the 2D boxes in LDS, formed at every step
struct CmBoxCost {
  const FmBox* gb;
  const FmBox* tb;
  typedef FmBox Row;
  __device__ __forceinline__ void bind(const FmBox* g, const FmBox* t) {
    gb = g;
    tb = t;
  }
  __device__ __forceinline__ Row row(bool tr, int i) const { return tr ? tb[i] : gb[i]; }
  __device__ __forceinline__ double cell(const Row& rb, bool tr, int j) const {
    return tr ? cm_c(gb[j], rb) : cm_c(rb, tb[j]);
  }
  __device__ __forceinline__ double c(int i, int j) const { return cm_c(gb[i], tb[j]); }
  __device__ __forceinline__ int col(int j) const { return j; }
  __device__ __forceinline__ void matched(int, int, bool) const {}
};

// what fm_assign searches: the gated cost of the functor's c, the rows being the smaller side (tr: the tracker side)
template <class F>
struct CmSearchCost {
  const F& cf;
  bool tr;
  double min_overlap;
  typedef typename F::Row Row;
  __device__ __forceinline__ Row row(int i) const { return cf.row(tr, i); }
  __device__ __forceinline__ double cell(const Row& rb, int j) const {
    return cm_cost(cf.cell(rb, tr, j), min_overlap);
  }
};

// One wave evaluates one frame of G ground-truth objects (from gsrc, attributes g_attr + 3 go) against T tracker
// columns (object cf.col(j) of tsrc / t_attr + 2 to) and D DontCare areas.  G, T <= FM_MAXN, D <= FM_MAXD.
template <class F>
__device__ __forceinline__ void cm_frame_body(F& cf, const FmBox* __restrict__ gsrc, const FmBox* __restrict__ tsrc,
                                              const FmBox* __restrict__ dsrc, int G, int T, int D, int go, int to,
                                              const int* __restrict__ g_attr, const int* __restrict__ t_attr,
                                              double min_overlap, double min_height, double max_truncation,
                                              double max_occlusion, double* __restrict__ fd, int* __restrict__ fi,
                                              int* __restrict__ gt_out) {
  constexpr int K = FM_MAXN / 64;
  __shared__ FmBox gb[FM_MAXN], tb[FM_MAXN], db[FM_MAXD];
  __shared__ double u[FM_MAXN], ov[FM_MAXN];
  __shared__ int row4col[FM_MAXN], col4row[FM_MAXN], path[FM_MAXN], mg[FM_MAXN], tval[FM_MAXN], tign[FM_MAXN];
  const int tid = threadIdx.x;
  cf.bind(gb, tb);
  const bool tr = G > T;  // rows are the smaller side
  const int R = tr ? T : G, C = tr ? G : T;
  for (int i = tid; i < G; i += 64) {
    gb[i] = gsrc[i];
    mg[i] = -1;
    ov[i] = 0.0;
  }
  for (int j = tid; j < T; j += 64) {
    tb[j] = tsrc[cf.col(j)];
    tval[j] = 0;
  }
  for (int d = tid; d < D; d += 64) db[d] = dsrc[d];
  fm_assign(R, C, tid, u, row4col, col4row, path, CmSearchCost<F>{cf, tr, min_overlap});

  // keep the assigned cells that pass the gate (`c < max_cost`, :488)
  for (int r = tid; r < R; r += 64) {
    const int c4 = col4row[r];
    if (c4 >= 0) {
      const int i = tr ? c4 : r, j = tr ? r : c4;
      const double c = cf.c(i, j);
      if (c <= min_overlap) {
        mg[i] = j;
        tval[j] = 1;
        ov[i] = 1.0 - c;
      }
    }
  }
  __syncthreads();

  // ignored trackers (:515-532): neighbouring class, height <= min_height or > 0.5 inside a DontCare box, while unmatched
  int n_itr = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int j = k * 64 + tid;
    bool ign = false;
    if (j < T && !tval[j]) {
      const FmBox b = tb[j];
      ign = t_attr[2 * (to + cf.col(j)) + 1] == 1 || fabs(b.y1 - b.y2) <= min_height;
      for (int d = 0; d < D && !ign; ++d) ign = fm_overlap(b, db[d], true) > 0.5;
    }
    if (j < T) tign[j] = ign ? 1 : 0;
    n_itr += fm_count(ign);
  }
  __syncthreads();

  // ground truth (:541-566) and the sums
  int nvalid = 0, ifn = 0, itp = 0, npairs = 0;
  double cost = 0.0, kept = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int i = k * 64 + tid;
    bool val = false, is_ifn = false, is_itp = false, pr = false;
    if (i < G) {
      const int j = mg[i];
      val = j >= 0;
      const int id = val ? t_attr[2 * (to + cf.col(j))] : -1;  // gg.tracker
      const int* a = g_attr + 3 * (go + i);
      const bool cond = (double)a[1] > max_occlusion || (double)a[0] > max_truncation || a[2] == 1;
      is_ifn = id < 0 && cond;
      is_itp = id >= 0 && cond;
      pr = is_itp && tign[j] > 0;
      gt_out[2 * (go + i)] = id;
      gt_out[2 * (go + i) + 1] = cond ? 1 : 0;
      cost += val ? ov[i] : 0.0;
      kept += (val && !is_itp) ? ov[i] : 0.0;
      cf.matched(i, j, val && !is_itp);
    }
    nvalid += fm_count(val);
    ifn += fm_count(is_ifn);
    itp += fm_count(is_itp);
    npairs += fm_count(pr);
  }
  cost = wave_sum_d(cost);
  kept = wave_sum_d(kept);
  if (tid == 0) {
    const int tmptp = nvalid - itp;
    fi[0] = nvalid;
    fi[1] = itp;
    fi[2] = G - nvalid - ifn;
    fi[3] = ifn;
    fi[4] = T - tmptp - n_itr - itp + npairs;
    fi[5] = n_itr;
    fd[0] = cost;
    fd[1] = tmptp != 0 ? kept / (double)tmptp : 1.0;
  }
}

// one lane per ground-truth trajectory (:698-743): traj_obj lists the trajectory's objects in frame order.  Level
// blockIdx.y reads gt_out + 2 nG level and writes traj_i + 4 NTr level.
__global__ __launch_bounds__(64) void cm_traj_kernel(const int* __restrict__ traj_off, const int* __restrict__ traj_obj,
                                                     int NTr, int nG, const int* __restrict__ gt_out,
                                                     int* __restrict__ traj_i) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= NTr) return;
  gt_out += (size_t)blockIdx.y * 2 * nG;
  traj_i += (size_t)blockIdx.y * 4 * NTr;
  const int b = traj_off[k], n = traj_off[k + 1] - b;
  int* o = traj_i + 4 * k;  // ignored, ID switches, fragments, 0 MT / 1 PT / 2 ML / -1 ignored
  bool ok = b >= 0 && n >= 1 && b <= nG - n;
  for (int p = 0; ok && p < n; ++p) ok = traj_obj[b + p] >= 0 && traj_obj[b + p] < nG;
  if (!ok) {
    o[0] = o[1] = o[2] = o[3] = -2;
    return;
  }
  auto gid = [&](int p) { return gt_out[2 * traj_obj[b + p]]; };
  auto ign = [&](int p) { return gt_out[2 * traj_obj[b + p] + 1] != 0; };
  int n_ign = 0, n_none = 0;
  for (int p = 0; p < n; ++p) {
    n_ign += ign(p) ? 1 : 0;
    n_none += gid(p) == -1 ? 1 : 0;
  }
  if (n_ign == n) {
    o[0] = 1; o[1] = 0; o[2] = 0; o[3] = -1;
    return;
  }
  if (n_none == n) {
    o[0] = 0; o[1] = 0; o[2] = 0; o[3] = 2;
    return;
  }
  int last_id = gid(0), tracked = last_id >= 0 ? 1 : 0, ids = 0, frag = 0;
  int prev = last_id, cur = n > 1 ? gid(1) : -1;
  for (int p = 1; p < n; ++p) {
    const int nxt = p + 1 < n ? gid(p + 1) : -1;
    if (ign(p)) {
      last_id = -1;
    } else {
      if (last_id != cur && last_id != -1 && cur != -1 && prev != -1) ++ids;
      if (p < n - 1 && prev != cur && last_id != -1 && cur != -1 && nxt != -1) ++frag;
      if (cur != -1) {
        ++tracked;
        last_id = cur;
      }
    }
    if (p == n - 1) {  // the last-frame rule (:729)
      if (prev != cur && last_id != -1 && cur != -1 && !ign(p)) ++frag;
    } else {
      prev = cur;
      cur = nxt;
    }
  }
  const double ratio = (double)tracked / (double)(n - n_ign);
  o[0] = 0;
  o[1] = ids;
  o[2] = frag;
  o[3] = ratio > 0.8 ? 0 : (ratio < 0.2 ? 2 : 1);
}

// one wave per sequence and level: lane-strided partial sums in index order, then a butterfly - the same order
// whatever else the call holds
__global__ __launch_bounds__(64) void cm_seq_kernel(const int* __restrict__ seq_off, int S, int NF, int NTr,
                                                    const double* __restrict__ frame_d,
                                                    const int* __restrict__ frame_i, const int* __restrict__ traj_i,
                                                    double* __restrict__ seq_d, int* __restrict__ seq_i) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const size_t lv = blockIdx.y;
  frame_d += lv * 2 * NF;
  frame_i += lv * 6 * NF;
  traj_i += lv * 4 * NTr;
  seq_d += lv * 2 * (S + 1);
  seq_i += lv * CM_SEQ_INTS * (S + 1);
  const int f0 = seq_off[2 * s], f1 = seq_off[2 * s + 2], t0 = seq_off[2 * s + 1], t1 = seq_off[2 * s + 3];
  int a[CM_SEQ_INTS];
#pragma unroll
  for (int q = 0; q < CM_SEQ_INTS; ++q) a[q] = 0;
  double cost = 0.0, modp = 0.0;
  for (int f = f0 + lane; f < f1; f += 64) {
#pragma unroll
    for (int q = 0; q < 6; ++q) a[q] += frame_i[6 * f + q];
    cost += frame_d[2 * f];
    modp += frame_d[2 * f + 1];
  }
  for (int k = t0 + lane; k < t1; k += 64) {
    const int ig = traj_i[4 * k], cat = traj_i[4 * k + 3];
    a[6] += traj_i[4 * k + 1];
    a[7] += traj_i[4 * k + 2];
    a[8] += cat == 0 ? 1 : 0;
    a[9] += cat == 1 ? 1 : 0;
    a[10] += cat == 2 ? 1 : 0;
    a[11] += ig == 1 ? 1 : 0;
  }
#pragma unroll
  for (int q = 0; q < CM_SEQ_INTS; ++q) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a[q] += __shfl_xor(a[q], o);
  }
  cost = wave_sum_d(cost);
  modp = wave_sum_d(modp);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < CM_SEQ_INTS; ++q) seq_i[CM_SEQ_INTS * s + q] = a[q];
    seq_d[2 * s] = cost;
    seq_d[2 * s + 1] = modp;
  }
}

// totals into row S of level blockIdx.x: the sequences in order
__global__ __launch_bounds__(64) void cm_total_kernel(int S, double* __restrict__ seq_d, int* __restrict__ seq_i) {
  const int lane = threadIdx.x;
  seq_d += (size_t)blockIdx.x * 2 * (S + 1);
  seq_i += (size_t)blockIdx.x * CM_SEQ_INTS * (S + 1);
  if (lane < CM_SEQ_INTS) {
    int a = 0;
    for (int s = 0; s < S; ++s) a += seq_i[CM_SEQ_INTS * s + lane];
    seq_i[CM_SEQ_INTS * S + lane] = a;
  } else if (lane < CM_SEQ_INTS + 2) {
    const int q = lane - CM_SEQ_INTS;
    double a = 0.0;
    for (int s = 0; s < S; ++s) a += seq_d[2 * s + q];
    seq_d[2 * S + q] = a;
  }
}

}  // namespace
