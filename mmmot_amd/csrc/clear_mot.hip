// CLEAR-MOT evaluation of tracked sequences (reference kitti_devkit/evaluate_tracking.py compute3rdPartyMetrics
// :393-792) in four launches: one workgroup (one wave) per FRAME for the Hungarian association and the per-frame
// counters, one lane per ground-truth TRAJECTORY for ID switches / fragments / MT-PT-ML, one workgroup per SEQUENCE
// for the sums, one lane for the totals.  Frames are independent of each other (the reference's last_ids / ids / fr
// bookkeeping of :654-669 feeds nothing) and so are trajectories.
//
// Frame: with c = 1 - IoU (boxoverlap :364-391 in its operation order, fp64, no contraction) a cell is valid where
// c <= min_overlap.  Munkres on the reference's zero-padded matrix (1e9 in the invalid cells) assigns min(G, T) rows
// and thereby takes as many valid cells as a matching can hold and among those the smallest sum of c.  Here the
// shortest-augmenting-path search of csrc/frame_match.h assigns every row of the smaller side at cost c - CM_K (valid)
// or 0 (invalid): CM_K = 128 outweighs any sum of c a frame can hold (<= 64), so one more valid cell always wins; rows
// that end on an invalid cell are dropped afterwards, which is what `c < max_cost` does there.  The gains are formed from the
// boxes in LDS at every step.  Ties between equal-cost matchings go to the smallest column index, which need not be
// munkres's choice.
//
// Ignore logic (:506-566) and counters (:571-611) as written, including the two comparisons that look at the matched
// tracker's ID instead of at "is matched" (a GT whose partner has a negative ID takes the false-negative branch) and
// nignoredpairs, which is always 0 because a matched tracker is never ignored (tracker IDs are unique per frame: the
// loader refuses a file where they are not).
#include "cm_search.h"  // the frame body (association, ignore logic, counters), trajectory / sequence / total kernels

namespace {

__global__ __launch_bounds__(64) void cm_frame_kernel(const double* __restrict__ boxes, int nG, int nT, int nD,
                                                      const int* __restrict__ frames, const int* __restrict__ g_attr,
                                                      const int* __restrict__ t_attr, double min_overlap,
                                                      double min_height, double max_truncation, double max_occlusion,
                                                      double* __restrict__ frame_d, int* __restrict__ frame_i,
                                                      int* __restrict__ gt_out) {
  const int f = blockIdx.x;
  const FmFrame fr = fm_frame(frames + 6 * f, nG, nT, nD);
  if (!fr.ok) {
    cm_frame_mark(frame_d + 2 * f, frame_i + 6 * f);
    return;
  }
  const int go = fr.go, G = fr.G, to = fr.to, T = fr.T, dof = fr.dof, D = fr.D;
  CmBoxCost cf;
  cm_frame_body(cf, (const FmBox*)boxes + go, (const FmBox*)boxes + nG + to, (const FmBox*)boxes + nG + nT + dof, G, T,
                D, go, to, g_attr, t_attr, min_overlap, min_height, max_truncation, max_occlusion, frame_d + 2 * f,
                frame_i + 6 * f, gt_out);
}

}  // namespace

extern "C" int mmmot_clear_mot(const double* boxes, int nG, int nT, int nD, const int* frames, int NF,
                               const int* g_attr, const int* t_attr, const int* traj_off, const int* traj_obj, int NTr,
                               const int* seq_off, int S, double min_overlap, double min_height, double max_truncation,
                               double max_occlusion, double* frame_d, int* frame_i, int* gt_out, int* traj_i,
                               double* seq_d, int* seq_i, void* stream) {
  if (nG < 0 || nT < 0 || nD < 0 || NF < 0 || NTr < 0 || S < 1) return MMMOT_EINVAL;
  if (!seq_off || !seq_d || !seq_i) return MMMOT_EINVAL;
  if (NF > 0 && (!frames || !frame_d || !frame_i)) return MMMOT_EINVAL;
  if (nG + nT + nD > 0 && !boxes) return MMMOT_EINVAL;
  if (nG > 0 && (!g_attr || !gt_out || !traj_obj)) return MMMOT_EINVAL;
  if (nT > 0 && !t_attr) return MMMOT_EINVAL;
  if (NTr > 0 && (!traj_off || !traj_i)) return MMMOT_EINVAL;
  if ((((uintptr_t)boxes) | ((uintptr_t)frame_d) | ((uintptr_t)seq_d)) & 7u) return MMMOT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (NF > 0)
    hipLaunchKernelGGL(cm_frame_kernel, dim3(NF), dim3(64), 0, st, boxes, nG, nT, nD, frames, g_attr, t_attr,
                       min_overlap, min_height, max_truncation, max_occlusion, frame_d, frame_i, gt_out);
  if (NTr > 0)
    hipLaunchKernelGGL(cm_traj_kernel, dim3((NTr + 63) / 64), dim3(64), 0, st, traj_off, traj_obj, NTr, nG, gt_out,
                       traj_i);
  hipLaunchKernelGGL(cm_seq_kernel, dim3(S), dim3(64), 0, st, seq_off, S, NF, NTr, frame_d, frame_i, traj_i, seq_d,
                     seq_i);
  hipLaunchKernelGGL(cm_total_kernel, dim3(1), dim3(64), 0, st, S, seq_d, seq_i);
  return mm_check(hipGetLastError());
}
