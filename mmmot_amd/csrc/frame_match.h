// What the fp64 frame evaluators share (clear_mot.hip and mot3d.hip through cm_search.h, hota.hip): the 2D box and its
// overlap, the per-frame limits, the check of a frame-table row, and the one-wave shortest-augmenting-path assignment.
// Included by one .hip file each; everything is file-local.
#pragma once
#include "common.h"

#define FM_MAXN 128  // ground-truth or tracker boxes per frame (CLEAR_MOT_MAX_BOXES)
#define FM_MAXD 64   // DontCare boxes per frame (CLEAR_MOT_MAX_DONTCARE)

namespace {

struct FmBox {
  double x1, y1, x2, y2;
};

// boxoverlap(a, b, "union") / (a, b, "a"): every product, sum and quotient rounded on its own
__device__ __forceinline__ double fm_overlap(const FmBox& a, const FmBox& b, bool over_a) {
#pragma clang fp contract(off)
  const double x1 = fmax(a.x1, b.x1), y1 = fmax(a.y1, b.y1), x2 = fmin(a.x2, b.x2), y2 = fmin(a.y2, b.y2);
  const double w = x2 - x1, h = y2 - y1;
  if (w <= 0.0 || h <= 0.0) return 0.0;
  const double inter = w * h;
  const double aarea = (a.x2 - a.x1) * (a.y2 - a.y1);
  if (over_a) return inter / aarea;
  const double barea = (b.x2 - b.x1) * (b.y2 - b.y1);
  return inter / (aarea + barea - inter);
}

// the smaller value, and among equal values the smaller column
__device__ __forceinline__ void fm_better(double& bv, int& bj, double ov, int oj) {
  if (ov < bv || (ov == bv && oj < bj)) {
    bv = ov;
    bj = oj;
  }
}

__device__ __forceinline__ int fm_count(bool p) { return __popcll(__ballot(p)); }

struct FmFrame {
  int go, G, to, T, dof, D;
  bool ok;  // inside the contract and the sections
};

// row fr of the frame table (first ground-truth box, G, first tracker box, T, first DontCare area, D), checked against
// the limits and the section sizes
__device__ __forceinline__ FmFrame fm_frame(const int* __restrict__ fr, int nG, int nT, int nD) {
  FmFrame r;
  r.go = fr[0], r.G = fr[1], r.to = fr[2], r.T = fr[3], r.dof = fr[4], r.D = fr[5];
  r.ok = !(r.G < 0 || r.T < 0 || r.D < 0 || r.G > FM_MAXN || r.T > FM_MAXN || r.D > FM_MAXD || r.go < 0 || r.to < 0 ||
           r.dof < 0 || r.go > nG - r.G || r.to > nT - r.T || r.dof > nD - r.D);
  return r;
}

// The assignment of one frame by ONE wave (tid = lane), two columns a lane: rows 0 .. R-1 are all assigned at the
// smallest sum of cost over (row, column); R <= C <= FM_MAXN and every cost is finite.  Shortest augmenting paths, one
// row after the other; ties between equal reduced costs go to the smaller column.  col4row[r] is row r's column.  u,
// row4col, col4row and path are the caller's LDS arrays of FM_MAXN entries, initialised here.  The cost object provides
//   F::Row                 what the search keeps of its current row
//   Row row(int i)         fetched once per step of the search
//   double cell(row, j)    the cost of (row, column j), evaluated per column
template <class F>
__device__ __forceinline__ void fm_assign(int R, int C, int tid, double* u, int* row4col, int* col4row, int* path,
                                          const F& cost) {
#pragma clang fp contract(off)  // a cost that ends in a product must not fuse into the reduced cost's sum
  constexpr int K = FM_MAXN / 64;
  for (int r = tid; r < R; r += 64) {
    u[r] = 0.0;
    col4row[r] = -1;
  }
  for (int j = tid; j < C; j += 64) {
    row4col[j] = -1;
    path[j] = -1;
  }
  __syncthreads();
  double v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = 0.0;
  for (int cur = 0; cur < R; ++cur) {
    double sp[K];
#pragma unroll
    for (int k = 0; k < K; ++k) sp[k] = INFINITY;
    unsigned scanned = 0;
    double minv = 0.0;
    int i = cur, sink = -1;
    for (;;) {
      const double ui = u[i];
      const typename F::Row rb = cost.row(i);
      double bv = INFINITY;
      int bj = 0x7fffffff;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int j = k * 64 + tid;
        if (j < C && !((scanned >> k) & 1u)) {
          const double r = minv + cost.cell(rb, j) - ui - v[k];
          if (r < sp[k]) {
            sp[k] = r;
            path[j] = i;
          }
          if (sp[k] < bv) {
            bv = sp[k];
            bj = j;
          }
        }
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) fm_better(bv, bj, __shfl_xor(bv, o), __shfl_xor(bj, o));
      if (bj >= C) break;  // cannot happen: every cost is finite and C >= R
      minv = bv;
      if ((bj & 63) == tid) scanned |= 1u << (bj >> 6);
      const int nxt = row4col[bj];
      if (nxt < 0) {
        sink = bj;
        break;
      }
      i = nxt;
    }
    if (sink >= 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int j = k * 64 + tid;
        if ((scanned >> k) & 1u) {
          const double d = minv - sp[k];
          v[k] -= d;
          if (j != sink) u[row4col[j]] += d;
        }
      }
      if (tid == 0) u[cur] += minv;
    }
    __syncthreads();
    if (tid == 0 && sink >= 0) {
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
}

}  // namespace
