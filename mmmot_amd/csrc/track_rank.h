// Shared by the track ID kernels (track_ids.hip: pairs, track_chain_ids.hip: windows of 2 .. 8 frames): the frame limit
// of the sequence state and the workgroup-wide rank that hands out "the next free ID in detection order".
#pragma once
#include "common.h"

#define TK_MAXN 512

namespace {

// exclusive count of `p` over the threads before this one, and the workgroup's total (every thread calls it)
template <int NW>
__device__ __forceinline__ int tk_rank(bool p, int& total, int* red) {
  const unsigned long long b = __ballot(p);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = __popcll(b & ((1ull << lane) - 1ull));
  if (NW == 1) {
    total = __popcll(b);
    return r;
  }
  if (lane == 0) red[wv] = __popcll(b);
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const int c = red[w];
    before += w < wv ? c : 0;
    all += c;
  }
  __syncthreads();  // red is free for the next call
  total = all;
  return r + before;
}

}  // namespace
