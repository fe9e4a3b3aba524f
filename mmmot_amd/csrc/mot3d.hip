// 3D MOT evaluation (DESIGN.md section 13 "3D / AMOTA"; restated in tests/mot3d_ref.py): the CLEAR-MOT evaluation of
// csrc/cm_search.h with c = 1 - overlap read from a per-frame table, at levels + 1 operating points.
//
// Table: one workgroup per frame, lanes over the G x T cells.  A cell clips the ground-truth footprint (a quadrilateral
// in the (x, z) plane, corners formed on the host) by the four edges of the tracker footprint (Sutherland-Hodgman, at
// most 8 vertices), takes the shoelace sum about vertex 0, and with the height overlap forms IoU3D or IoUbev; fp64,
// no contraction, the operation order of tests/mot3d_ref.py.  Each lane keeps its two 8-vertex polygons in LDS
// ([buffer][slot][lane]: 16 KB, conflict-free), so that the running vertex count indexes LDS and not scratch.  Mode '2d'
// fills the table with cm_c of the 2D boxes.
//
// Frame kernel, grid (frame, level): the wave reads thr[level] (level `levels` is pass A: -inf), lists the tracker
// columns whose track score is >= thr in LDS, in order, and runs cm_frame_body on those columns with the table cost.
// Pass A also leaves, per ground-truth object, the track score of its partner where the pair is a true positive that
// is not ignored (-inf elsewhere); sorted descending by the caller, m3_thr_kernel picks the thresholds of the levels
// from it.  No floating-point atomics anywhere.
#include "cm_search.h"

#define M3_BOX 12  // doubles per 3D box: corners (x, z) x 4, y - h, y, w l, h w l

namespace {

// area of the intersection of the footprints a (subject) and b (clip), 8 doubles each.  Both run the same way round
// (the host forms them so), with the inside of an edge A -> B where ex (Pz - Az) - ez (Px - Ax) <= 0.
__device__ __forceinline__ double m3_clip_area(const double* __restrict__ a, const double* __restrict__ b,
                                               double (*px)[8][64], double (*pz)[8][64], int tid) {
#pragma clang fp contract(off)
  double bx[4], bz[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    px[0][k][tid] = a[2 * k];
    pz[0][k][tid] = a[2 * k + 1];
    bx[k] = b[2 * k];
    bz[k] = b[2 * k + 1];
  }
  int n = 4, src = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const double ax = bx[e], az = bz[e];
    const double ex = bx[(e + 1) & 3] - ax, ez = bz[(e + 1) & 3] - az;
    const int dst = src ^ 1;
    int m = 0;
    if (n > 0) {
      double sx = px[src][n - 1][tid], sz = pz[src][n - 1][tid];
      double ds = ex * (sz - az) - ez * (sx - ax);
      for (int k = 0; k < n; ++k) {
        const double qx = px[src][k][tid], qz = pz[src][k][tid];
        const double de = ex * (qz - az) - ez * (qx - ax);
        const bool in_e = de <= 0.0, in_s = ds <= 0.0;
        if (in_e != in_s && m < 8) {  // the edge S -> E crosses the line
          const double t = ds / (ds - de);
          px[dst][m][tid] = sx + t * (qx - sx);
          pz[dst][m][tid] = sz + t * (qz - sz);
          ++m;
        }
        if (in_e && m < 8) {
          px[dst][m][tid] = qx;
          pz[dst][m][tid] = qz;
          ++m;
        }
        sx = qx;
        sz = qz;
        ds = de;
      }
    }
    n = m;
    src = dst;
  }
  if (n < 3) return 0.0;
  const double x0 = px[src][0][tid], z0 = pz[src][0][tid];
  double s = 0.0;
  for (int k = 1; k + 1 < n; ++k) {
    const double ux = px[src][k][tid] - x0, uz = pz[src][k][tid] - z0;
    const double vx = px[src][k + 1][tid] - x0, vz = pz[src][k + 1][tid] - z0;
    s = s + (ux * vz - vx * uz);
  }
  return 0.5 * fabs(s);
}

// c = 1 - IoU3D (bev: 1 - IoUbev) of the boxes g and t (M3_BOX doubles each)
__device__ __forceinline__ double m3_c(const double* __restrict__ g, const double* __restrict__ t, bool bev,
                                       double (*px)[8][64], double (*pz)[8][64], int tid) {
#pragma clang fp contract(off)
  const double A = m3_clip_area(g, t, px, pz, tid);
  double iou = 0.0;
  if (A > 0.0) {
    if (bev) {
      iou = A / ((g[10] + t[10]) - A);
    } else {
      const double H = fmin(g[9], t[9]) - fmax(g[8], t[8]);
      if (H > 0.0) {
        const double I = A * H;
        iou = I / ((g[11] + t[11]) - I);
      }
    }
  }
  return 1.0 - iou;
}

// the frame's cells fit the table?
__device__ __forceinline__ bool m3_cells_ok(int off, int G, int T, long long cells) {
  return off >= 0 && (long long)off + (long long)G * T <= cells;
}

// mode 0: '3d', 1: 'bev', 2: '2d'
__global__ __launch_bounds__(64) void m3_table_kernel(const double* __restrict__ boxes,
                                                      const double* __restrict__ box3d, int nG, int nT, int nD,
                                                      const int* __restrict__ frames,
                                                      const int* __restrict__ cell_off, long long cells, int mode,
                                                      double* __restrict__ table) {
  __shared__ double px[2][8][64], pz[2][8][64];
  const int f = blockIdx.x, tid = threadIdx.x;
  const FmFrame fr = fm_frame(frames + 6 * f, nG, nT, nD);
  if (!fr.ok) return;
  const int go = fr.go, G = fr.G, to = fr.to, T = fr.T;
  const int off = cell_off[f];
  if (!m3_cells_ok(off, G, T, cells)) return;
  double* tab = table + off;
  const int n = G * T;
  for (int idx = tid; idx < n; idx += 64) {
    const int i = idx / T, j = idx - i * T;
    double c;
    if (mode == 2) {
      c = cm_c(((const FmBox*)boxes)[go + i], ((const FmBox*)boxes)[nG + to + j]);
    } else {
      c = m3_c(box3d + (size_t)M3_BOX * (go + i), box3d + (size_t)M3_BOX * (nG + to + j), mode == 1, px, pz, tid);
    }
    tab[idx] = c;
  }
}

// the cost from the frame's table, over the kept columns
struct M3TableCost {
  const double* tab;  // [G][T0]
  int T0;
  const int* kept;      // LDS: column -> tracker object of the frame
  const double* sigma;  // track score of the frame's tracker objects
  double* msig;         // pass A: matched score per ground-truth object of the frame, or null
  typedef const double* Row;
  __device__ __forceinline__ void bind(const FmBox*, const FmBox*) const {}  // the 2D boxes are not the cost here
  __device__ __forceinline__ Row row(bool tr, int i) const { return tr ? tab + kept[i] : tab + (size_t)i * T0; }
  __device__ __forceinline__ double cell(Row rb, bool tr, int j) const {
    return tr ? rb[(size_t)j * T0] : rb[kept[j]];
  }
  __device__ __forceinline__ double c(int i, int j) const { return tab[(size_t)i * T0 + kept[j]]; }
  __device__ __forceinline__ int col(int j) const { return kept[j]; }
  __device__ __forceinline__ void matched(int i, int j, bool tp) const {
    if (msig) msig[i] = tp ? sigma[kept[j]] : -INFINITY;
  }
};

__global__ __launch_bounds__(64) void m3_frame_kernel(const double* __restrict__ boxes, int nG, int nT, int nD,
                                                      const int* __restrict__ frames, int NF,
                                                      const int* __restrict__ cell_off, long long cells,
                                                      const double* __restrict__ table,
                                                      const double* __restrict__ sigma,
                                                      const double* __restrict__ thr, int levels, int lev0,
                                                      const int* __restrict__ g_attr, const int* __restrict__ t_attr,
                                                      double gate, double min_height, double max_truncation,
                                                      double max_occlusion, double* __restrict__ msig,
                                                      double* __restrict__ frame_d, int* __restrict__ frame_i,
                                                      int* __restrict__ gt_out) {
  __shared__ int kept[FM_MAXN];
  const int f = blockIdx.x, tid = threadIdx.x, level = lev0 + blockIdx.y;
  const FmFrame fr = fm_frame(frames + 6 * f, nG, nT, nD);
  double* fd = frame_d + 2 * ((size_t)level * NF + f);
  int* fi = frame_i + 6 * ((size_t)level * NF + f);
  if (!fr.ok || !m3_cells_ok(cell_off[f], fr.G, fr.T, cells)) {
    cm_frame_mark(fd, fi);
    return;
  }
  const int go = fr.go, G = fr.G, to = fr.to, T0 = fr.T, dof = fr.dof, D = fr.D;
  const double th = level == levels ? -INFINITY : thr[level];
  int T = 0;
#pragma unroll
  for (int k = 0; k < FM_MAXN / 64; ++k) {
    const int j = k * 64 + tid;
    const bool keep = j < T0 && sigma[to + j] >= th;
    const unsigned long long mask = __ballot(keep);
    if (keep) kept[T + __popcll(mask & ((1ull << tid) - 1ull))] = j;
    T += __popcll(mask);
  }
  __syncthreads();
  M3TableCost cf;
  cf.tab = table + cell_off[f];
  cf.T0 = T0;
  cf.kept = kept;
  cf.sigma = sigma + to;
  cf.msig = level == levels ? msig + go : nullptr;
  cm_frame_body(cf, (const FmBox*)boxes + go, (const FmBox*)boxes + nG + to, (const FmBox*)boxes + nG + nT + dof, G, T,
                D, go, to, g_attr, t_attr, gate, min_height, max_truncation, max_occlusion, fd, fi,
                gt_out + (size_t)level * 2 * nG);
}

// thresholds of the sweep from pass A: sorted = the matched scores, descending, -inf where an object has none;
// tot = pass A's totals row.  need_k = ceil(k n_gt / levels); level k is reachable when n_gt > 0 and need_k <= n.
__global__ __launch_bounds__(64) void m3_thr_kernel(const double* __restrict__ sorted, int nG,
                                                    const int* __restrict__ tot, int levels, double* __restrict__ thr,
                                                    int* __restrict__ reach) {
  const int lane = threadIdx.x;
  int n = 0;
  for (int i = lane; i < nG; i += 64) n += sorted[i] > -INFINITY ? 1 : 0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o);
  const long long n_gt = (long long)nG - tot[1] - tot[3];
  for (int k = lane + 1; k <= levels; k += 64) {
    const long long need = (k * n_gt + levels - 1) / levels;
    const bool ok = n_gt > 0 && need >= 1 && need <= n;
    thr[k - 1] = ok ? sorted[need - 1] : INFINITY;
    reach[k - 1] = ok ? 1 : 0;
  }
}

}  // namespace

extern "C" int mmmot_mot3d(const double* boxes, const double* box3d, const double* sigma, int nG, int nT, int nD,
                           const int* frames, const int* cell_off, int NF, const int* g_attr, const int* t_attr,
                           const int* traj_off, const int* traj_obj, int NTr, const int* seq_off, int S, int mode,
                           int levels, int phase, double gate, double min_height, double max_truncation,
                           double max_occlusion, double* table, long long cells, double* msig, double* frame_d,
                           int* frame_i, int* gt_out, int* traj_i, double* seq_d, int* seq_i, double* thr, int* reach,
                           void* stream) {
  if (nG < 0 || nT < 0 || nD < 0 || NF < 0 || NTr < 0 || S < 1 || cells < 0 || cells >= (1ll << 31)) return MMMOT_EINVAL;
  if (mode < 0 || mode > 2 || levels < 0 || levels > 1024 || phase < 0 || phase > 1) return MMMOT_EINVAL;
  if (phase == 1 && levels == 0) return MMMOT_EINVAL;
  if (!seq_off || !seq_d || !seq_i) return MMMOT_EINVAL;
  if (NF > 0 && (!frames || !cell_off || !frame_d || !frame_i)) return MMMOT_EINVAL;
  if (nG + nT + nD > 0 && !boxes) return MMMOT_EINVAL;
  if (mode != 2 && nG + nT > 0 && !box3d) return MMMOT_EINVAL;
  if (cells > 0 && !table) return MMMOT_EINVAL;
  if (nG > 0 && (!g_attr || !gt_out || !traj_obj || !msig)) return MMMOT_EINVAL;
  if (nT > 0 && (!t_attr || !sigma)) return MMMOT_EINVAL;
  if (NTr > 0 && (!traj_off || !traj_i)) return MMMOT_EINVAL;
  if (levels > 0 && (!thr || !reach)) return MMMOT_EINVAL;
  if ((((uintptr_t)boxes) | ((uintptr_t)box3d) | ((uintptr_t)sigma) | ((uintptr_t)table) | ((uintptr_t)msig) |
       ((uintptr_t)frame_d) | ((uintptr_t)seq_d) | ((uintptr_t)thr)) & 7u)
    return MMMOT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  // phase 0: the table and pass A (level `levels`); phase 1: the thresholds and the levels 0 .. levels - 1
  const int lev0 = phase == 0 ? levels : 0, nlev = phase == 0 ? 1 : levels;
  const size_t L0 = (size_t)lev0;
  if (phase == 0) {
    if (NF > 0 && cells > 0)
      hipLaunchKernelGGL(m3_table_kernel, dim3(NF), dim3(64), 0, st, boxes, box3d, nG, nT, nD, frames, cell_off, cells,
                         mode, table);
  } else {
    hipLaunchKernelGGL(m3_thr_kernel, dim3(1), dim3(64), 0, st, (const double*)msig, nG,
                       (const int*)(seq_i + CM_SEQ_INTS * ((size_t)levels * (S + 1) + S)), levels, thr, reach);
  }
  if (NF > 0)
    hipLaunchKernelGGL(m3_frame_kernel, dim3(NF, nlev), dim3(64), 0, st, boxes, nG, nT, nD, frames, NF, cell_off, cells,
                       (const double*)table, sigma, (const double*)thr, levels, lev0, g_attr, t_attr, gate, min_height,
                       max_truncation, max_occlusion, msig, frame_d, frame_i, gt_out);
  if (NTr > 0)
    hipLaunchKernelGGL(cm_traj_kernel, dim3((NTr + 63) / 64, nlev), dim3(64), 0, st, traj_off, traj_obj, NTr, nG,
                       (const int*)(gt_out + L0 * 2 * nG), traj_i + L0 * 4 * NTr);
  hipLaunchKernelGGL(cm_seq_kernel, dim3(S, nlev), dim3(64), 0, st, seq_off, S, NF, NTr,
                     (const double*)(frame_d + L0 * 2 * NF), (const int*)(frame_i + L0 * 6 * NF),
                     (const int*)(traj_i + L0 * 4 * NTr), seq_d + L0 * 2 * (S + 1), seq_i + L0 * CM_SEQ_INTS * (S + 1));
  hipLaunchKernelGGL(cm_total_kernel, dim3(nlev), dim3(64), 0, st, S, seq_d + L0 * 2 * (S + 1),
                     seq_i + L0 * CM_SEQ_INTS * (S + 1));
  return mm_check(hipGetLastError());
}
