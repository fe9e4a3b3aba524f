// The tables of tracked sequences and the links along a track ID, shared by csrc/fill_tracks.hip
// and csrc/smooth_tracks.hip (section 12b): det [L][12], ids [L], frame_start [F+1], frame_no [F], seq_start [S+1] as
// include/mmmot_hip.h describes them for mmmot_fill_tracks.  Integer work only; each source wraps these in kernels of
// its own.
#pragma once
#include "common.h"

// last t in [0, n) with tab[t] <= v (t = 0 when there is none): the frame of a detection, the sequence of a frame.  Empty
// frames / sequences share their start with the next one and are skipped.  Stays inside [0, n) whatever the table holds.
__device__ __forceinline__ int ft_last_le(const int* __restrict__ tab, int n, int v) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid] <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Table entry i of max(F, S): the shape of seq_start / frame_start (a violation sets *bad and stops the whole call,
// because every later index is derived from them) and the order of the frame numbers (a violation gives its sequence
// MMMOT_FILL_ECONTRACT in info[4 s]).
__device__ __forceinline__ void ft_check_entry(int i, const int* __restrict__ frame_start,
                                               const int* __restrict__ frame_no, const int* __restrict__ seq_start,
                                               int L, int F, int S, int* __restrict__ bad_flag, int* __restrict__ info) {
  bool bad = false;
  if (i < S) {
    const int a = seq_start[i], b = seq_start[i + 1];
    bad = a < 0 || a > b || b > F || (i == 0 && a != 0) || (i == S - 1 && b != F);
  }
  if (i < F) {
    const int a = frame_start[i], b = frame_start[i + 1];
    bad = bad || a < 0 || a > b || b > L || (i == 0 && a != 0) || (i == F - 1 && b != L);
  }
  if (bad) atomicOr(bad_flag, 1);
  if (i + 1 < F && frame_no[i] >= frame_no[i + 1]) {
    const int s = ft_last_le(seq_start, S, i);
    if (i + 1 < seq_start[s + 1]) atomicOr(&info[4 * s], MMMOT_FILL_ECONTRACT);
  }
}

// does another detection of listed frame pa carry the ID of detection i?
__device__ __forceinline__ bool ft_dup_in_frame(const int* __restrict__ ids, const int* __restrict__ frame_start, int pa,
                                                int i, int id) {
  bool dup = false;
  for (int c = frame_start[pa]; c < frame_start[pa + 1]; ++c) dup = dup || (c != i && ids[c] == id);
  return dup;
}

// the next detection of `id` behind listed frame pa in the frames [pa + 1, e): its index (-1: none) and its frame in pb.
// The scan ends at the first hit, so only the last observation of a track walks to the sequence end.
__device__ __forceinline__ int ft_successor(const int* __restrict__ ids, const int* __restrict__ frame_start, int pa,
                                            int e, int id, int& pb) {
  int sj = -1;
  pb = -1;
  for (int q = pa + 1; q < e && sj < 0; ++q)
    for (int c = frame_start[q]; c < frame_start[q + 1]; ++c)
      if (ids[c] == id) {
        sj = c, pb = q;
        break;
      }
  return sj;
}
