// What the kernels behind mmmot_gemm_ares share (gemm_ares.hip, gemm_wres.hip, gemm_wreg.hip): the tile-table record
// and its two fetch forms, the register-only epilogue of a 64-row half tile, the zeros stand-in, and the launchers the
// dispatcher in gemm_ares.hip calls.  "Same arithmetic, same summation order, bit for bit" between these kernels holds
// because the pieces below exist once.
#pragma once
#include "ares_choice.h"
#include "common.h"

// stands in for absent bias / dbias / osc / osh rows (branch-free loads); the family's N <= 4096.  static: the library
// is not built with relocatable device code, every translation unit has its own.
static __device__ float ares_zeros[4096];

// ---- the tile-table record: the four words of a 128-row tile ----
struct AresTile {
  int row0, nrows, grp, dbrow;
};

// Fetch form 1 (gemm_ares_kernel, gemm_wres64_kernel): vector loads now, scalars later.  The table words are
// wave-uniform and those of tile t + 2 * gridDim.x are requested a whole tile before they are needed: a lookup at the
// tile switch is two dependent L2 round trips in front of the switch, with the matrix cores idle, and its vmcnt(0)
// also drains the loads that are meant to stay in flight.
__device__ __forceinline__ AresTile ares_tile_request(const mmmot_gemm_ares_args& a, int tt) {
  AresTile m;
  m.row0 = a.tile_row0[tt];
  m.nrows = a.tile_nrows[tt];
  // unconditional loads (an absent table reads tile_row0 instead, discarded in ares_tile_scalar): a conditional load
  // makes the number of loads in flight path-dependent and turns later counted waits into vmcnt(0)
  m.grp = (a.tile_group ? a.tile_group : a.tile_row0)[tt];
  m.dbrow = (a.dbias ? a.tile_dbrow : a.tile_row0)[tt];
  return m;
}
__device__ __forceinline__ AresTile ares_tile_scalar(const mmmot_gemm_ares_args& a, const AresTile& v) {
  AresTile m;
  m.row0 = __builtin_amdgcn_readfirstlane(v.row0);
  m.nrows = __builtin_amdgcn_readfirstlane(v.nrows);
  m.grp = a.tile_group ? __builtin_amdgcn_readfirstlane(v.grp) : 0;
  m.dbrow = a.dbias ? __builtin_amdgcn_readfirstlane(v.dbrow) : 0;
  return m;
}

// Fetch form 2 (gemm_wres64i_kernel, gemm_wreg128_kernel): hand-written scalar loads (mm_sload4, common.h).  These
// kernels store to global memory, so the compiler will not treat the tables as constant: it turns a plain read into a
// VECTOR load and then waits vmcnt(0) for it, i.e. for every request in flight, right after the requests were issued.
// Optional tables read a valid word (the tile's row0) and are replaced by 0 afterwards.
__device__ __forceinline__ AresTile ares_tile_sload(const mmmot_gemm_ares_args& a, int t) {
  const int* p0 = a.tile_row0 + t;
  const int* p1 = a.tile_nrows + t;
  const int* p2 = a.tile_group ? a.tile_group + t : p0;
  const int* p3 = a.dbias ? a.tile_dbrow + t : p0;
  int v0, v1, v2, v3;
  mm_sload4(p0, p1, p2, p3, v0, v1, v2, v3);
  AresTile m;
  m.row0 = v0;
  m.nrows = v1;
  m.grp = a.tile_group ? v2 : 0;
  m.dbrow = a.dbias ? v3 : 0;
  return m;
}

// ---- register-only epilogue of a wave's 64-row x 32-channel half tile: accumulator a0 holds rows 0-31, a1 rows 32-63.
// v = acc*oscale + cb is never formed: the sums are taken on the raw accumulators and the caller rescales
// (S = oscale*sum(acc) + n*cb, M2 = oscale^2 * M2(acc), relu(v*os+oh) = relu(acc*(oscale*os) + (cb*os+oh))); 3 VALU ops
// per value.  Per-lane order: a0, e = 0..15, then a1; then the half-wave exchange.
// A full half tile (64 rows) takes mm_sum32 / mm_m2_32 / mm_relu_sum32.  Otherwise element e of the 32-row block that
// starts at row R0 counts <=> R0 + mm_acc_row0(e) < lim, where lim = valid rows of the half tile - 4 * (lane >> 5):
// immediates against one register instead of 32 hoisted row indices.
template <int R0>
__device__ __forceinline__ float ares_sum_masked(const f32x16& acc, int lim, float s) {
#pragma unroll
  for (int e = 0; e < 16; ++e)
    if (R0 + mm_acc_row0(e) < lim) s += acc[e];
  return s;
}
template <int R0>
__device__ __forceinline__ float ares_m2_masked(const f32x16& acc, int lim, float mu, float s) {
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const float d = acc[e] - mu;
    if (R0 + mm_acc_row0(e) < lim) s = fmaf(d, d, s);
  }
  return s;
}
// (R0 = 0 on its own: the one-accumulator form of gemm_wreg128_kernel, which adds to a running sum)
template <int R0>
__device__ __forceinline__ float ares_relu_sum_masked(const f32x16& acc, int lim, float m1, float m0, float s) {
#pragma unroll
  for (int e = 0; e < 16; ++e)
    if (R0 + mm_acc_row0(e) < lim) s += fmaxf(fmaf(acc[e], m1, m0), 0.f);
  return s;
}

// sum (s1) and M2 centred on the half tile's own mean (s2) of the raw accumulators; inv_nsub = 1 / valid rows (0: none)
__device__ __forceinline__ void ares_half_stats(const f32x16& a0, const f32x16& a1, bool full, int lim, float inv_nsub,
                                                float& s1, float& s2) {
  if (full) {
    s1 = mm_sum32(a0, a1);
  } else {
    s1 = ares_sum_masked<32>(a1, lim, ares_sum_masked<0>(a0, lim, 0.f));
  }
  s1 = mm_xor32_sum(s1);
  float mu = s1 * inv_nsub;  // mean of the raw accumulators over the half tile
  // The mean is rounded here, once, and every element subtracts that value.  Left to itself the compiler contracts
  // single subtractions with the multiply, fma(-s1, inv_nsub, acc), depending on the code around this call (element 0
  // of the masked form in one kernel, none in another): kernels that share this code would not share its bits.
  asm("" : "+v"(mu));
  if (full) {
    s2 = mm_m2_32(a0, a1, mu);
  } else {
    s2 = ares_m2_masked<32>(a1, lim, mu, ares_m2_masked<0>(a0, lim, mu, 0.f));
  }
  s2 = mm_xor32_sum(s2);
}

// the consumer's column sum: sum over the valid rows of relu(acc * m1 + m0)
__device__ __forceinline__ float ares_half_relu_sum(const f32x16& a0, const f32x16& a1, bool full, int lim, float m1,
                                                    float m0) {
  float s3;
  if (full) {
    s3 = mm_relu_sum32(a0, a1, m1, m0);
  } else {
    s3 = ares_relu_sum_masked<32>(a1, lim, m1, m0, ares_relu_sum_masked<0>(a0, lim, m1, m0, 0.f));
  }
  return mm_xor32_sum(s3);
}

// ---- per-file launchers: grid sizing and the launch of the kernel mmmot_ares_choose picked (called by mmmot_gemm_ares
// after its argument checks) ----
int mmmot_gemm_wres64_launch(const mmmot_gemm_ares_args* a, int mode, bool waves, int n_cu, hipStream_t s);  // gemm_wres.hip
int mmmot_gemm_wreg128_launch(const mmmot_gemm_ares_args* a, int n_cu, hipStream_t s);                        // gemm_wreg.hip
