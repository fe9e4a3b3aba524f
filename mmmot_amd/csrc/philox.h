// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants), the
// counter-based generator behind the dropout mask of the LiDAR encoder.  Stateless: the four
// output words are a function of (counter, key) alone, so a forward and a backward kernel that never saw each other's
// grid regenerate the same mask from (seed, row, channel).
#pragma once
#include "common.h"

#define MM_PHILOX_M0 0xD2511F53u
#define MM_PHILOX_M1 0xCD9E8D57u
#define MM_PHILOX_W0 0x9E3779B9u
#define MM_PHILOX_W1 0xBB67AE85u

// ten rounds; the key is bumped by the Weyl constants between rounds (nine times)
__host__ __device__ __forceinline__ u32x4 mm_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                                           unsigned k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    // 32 x 32 -> 64-bit products: one v_mad_u64_u32 each gives the high and the low word
    const unsigned long long p0 = (unsigned long long)MM_PHILOX_M0 * c0;
    const unsigned long long p1 = (unsigned long long)MM_PHILOX_M1 * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1;
    c3 = (unsigned)p0;
    c0 = n0;
    c2 = n2;
    k0 += MM_PHILOX_W0;
    k1 += MM_PHILOX_W1;
  }
  return u32x4{c0, c1, c2, c3};
}

// The dropout words of the four channels c .. c + 3 (c a multiple of 4) of row r: element (r, c + e) is KEPT when
// word e >= threshold (unsigned compare).  counter = (r, c / 4, 0, 0), key = (seed low word, seed high word).
__host__ __device__ __forceinline__ u32x4 mm_dropout_words(unsigned long long seed, unsigned r, int c) {
  return mm_philox4x32_10(r, (unsigned)c >> 2, 0u, 0u, (unsigned)seed, (unsigned)(seed >> 32));
}

// keep(r, c + e) ? v[e] * scale : 0, for the words w of mm_dropout_words(seed, r, c)
__device__ __forceinline__ f32x4 mm_drop4(f32x4 v, u32x4 w, unsigned threshold, float scale) {
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = w[e] >= threshold ? v[e] * scale : 0.f;
  return v;
}
