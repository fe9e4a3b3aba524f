// Shared device helpers for the gfx950 kernels of libmmmot_hip.so.
// CDNA4 only: 64-lane wavefronts, v_mfma_f32_32x32x2_f32 (exact fp32 MFMA).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mmmot_hip.h"

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

#define MM_BM 128          // rows (positions) per workgroup tile
#define MM_BK 32           // reduction depth per LDS stage
#define MM_LDT (MM_BK + 4) // LDS row stride in floats: 144 B keeps ds_read_b128 conflict-free
#define MM_THREADS 256

static inline int mm_check(hipError_t e) { return e == hipSuccess ? MMMOT_OK : (int)e; }
static inline bool mm_al16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

// grid of a grid-stride launch of 256-thread workgroups over n items: one item per thread, at most 8192 workgroups
static inline int mm_grid256(long n) { return (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192); }

// CU count of the current device (one process drives one GPU); 0 when there is none.  A function-local static:
// initialised once, thread-safe (C++11).
static inline int mm_num_cu() {
  static const int n = [] {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    return (int)prop.multiProcessorCount;
  }();
  return n;
}

// XCD-aware bijective remap of a linear workgroup id: the dispatcher places
// workgroup b on XCD b % 8; give every XCD a contiguous chunk of logical ids so
// that tiles sharing an A panel hit the same 4 MiB L2.
__device__ __forceinline__ int mm_xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = bid & 7, slot = bid >> 3;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + slot;
}

// ---- hand-written memory primitives: LDS-DMA, counted waits, LDS reads and scalar loads the compiler does not track.
// Kernels that keep LDS-DMA in flight across their loops write these out because the compiler answers any load it can
// see - and any LDS read it cannot tell from a DMA destination - with s_waitcnt vmcnt(0).  A counted wait does not name
// the registers it guards: the consumers stay behind it only by the sched_barrier / asm ordering of the call site.

// 16 bytes per lane from global memory straight into LDS (global_load_lds_dwordx4: no VGPR staging, counted by vmcnt)
__device__ __forceinline__ void mm_dma16(const void* src, unsigned char* dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}

// at most N of this wave's vector-memory requests (loads, LDS-DMA, stores) still in flight
template <int N>
__device__ __forceinline__ void mm_wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// this wave's LDS reads (and scalar loads) landed
__device__ __forceinline__ void mm_lds_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// workgroup barrier that orders LDS accesses only (no vmcnt drain)
__device__ __forceinline__ void mm_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// LDS reads, written out: invisible to the compiler's wait insertion (pair with mm_lds_wait).  For a buffer that really is
// disjoint from every LDS-DMA destination in flight but lives in the same array (runtime offsets): a plain read of it is
// answered with vmcnt(0), which also waits for the wave's own global stores.
__device__ __forceinline__ unsigned mm_lds_addr(const void* p) {
  return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}
__device__ __forceinline__ void mm_lds_read32(unsigned addr, f32x4& a, f32x4& b) {  // 32 bytes at addr
  asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:16" : "=&v"(a), "=&v"(b) : "v"(addr));
}

// Four wave-uniform words (the tile-table entries of a work item) by s_load_dword, and their wait, as ONE asm block with
// early-clobber outputs: with the wait in a separate statement the compiler does not know the destination registers are
// pending and may schedule a scalar move / select on them in between.  A compiler-visible load would be
// answered with a wait that also drains the LDS-DMA in flight.
__device__ __forceinline__ void mm_sload4(const int* p0, const int* p1, const int* p2, const int* p3, int& v0, int& v1,
                                          int& v2, int& v3) {
  asm volatile(
      "s_load_dword %0, %4, 0x0\n\t"
      "s_load_dword %1, %5, 0x0\n\t"
      "s_load_dword %2, %6, 0x0\n\t"
      "s_load_dword %3, %7, 0x0\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&s"(v0), "=&s"(v1), "=&s"(v2), "=&s"(v3)
      : "s"(p0), "s"(p1), "s"(p2), "s"(p3)
      : "memory");
}

// One BK=32 stage of the wave-level MMA: the wave owns TM x TN 32x32 output
// tiles.  As / Bs are [rows][MM_LDT] fp32 with the reduction axis contiguous.
// Fragment mapping of v_mfma_f32_32x32x2_f32: lane l supplies A[i=l&31][k=l>>5]
// and B[k=l>>5][j=l&31].  Each lane reads 4 consecutive k with one
// ds_read_b128 (k = kc*8 + 4*(l>>5) + j) and issues 4 MFMAs; the pairing of k
// values inside one MFMA is (j, j+4), identical for A and B, so the sum is the
// plain dot product.
template <int TM, int TN>
__device__ __forceinline__ void mm_stage(const float* __restrict__ As, const float* __restrict__ Bs,
                                         f32x16 (&acc)[TM][TN], int a_row0, int b_row0, int lane) {
  const int lr = lane & 31;
  const int kh = (lane >> 5) * 4;
#pragma unroll
  for (int kc = 0; kc < MM_BK / 8; ++kc) {
    f32x4 a[TM], b[TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
      a[tm] = *reinterpret_cast<const f32x4*>(&As[(a_row0 + tm * 32 + lr) * MM_LDT + kc * 8 + kh]);
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
      b[tn] = *reinterpret_cast<const f32x4*>(&Bs[(b_row0 + tn * 32 + lr) * MM_LDT + kc * 8 + kh]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm][j], b[tn][j], acc[tm][tn], 0, 0, 0);
  }
}

// C/D mapping of the 32x32 MFMA: lane l, register e holds
// row = mm_acc_row0(e) + 4*(l>>5), col = l&31.  mm_acc_row0 is the lane-independent part (a compile-time constant in
// an unrolled loop over e).
constexpr int mm_acc_row0(int e) { return (e & 3) + 8 * (e >> 2); }
__device__ __forceinline__ int mm_acc_row(int e, int lane) { return mm_acc_row0(e) + 4 * (lane >> 5); }

// ---- register epilogues of a 64-row x 32-channel wave tile (two 32x32 accumulators; a lane holds 32 of its column's
// 64 rows, lane ^ 32 the other 32).  The half-wave exchange is v_permlane32_swap (gfx950), a VALU instruction, instead of
// the ds_bpermute behind __shfl_xor(.., 32) (an LDS round trip twice per channel block).  Measured and not adopted for
// the 32-value sums: packed fp32 (v_pk_add_f32 / v_pk_fma_f32) tree reductions - fewer instructions, no faster
// (tools/bench_ares.py A/B on one box: 0.44 ms sequential vs 0.47 ms packed, statistics pass of conv1).
// v_permlane32_swap_b32 a, b: the upper 32 lanes of a <-> the lower 32 lanes of b; returns the new {a, b}.  Inline
// assembly: with this toolchain (ROCm 7.2 clang) the second result of __builtin_amdgcn_permlane32_swap comes back equal
// to the first (probed on an MI355X), and the hazard recogniser does not see into inline assembly - the instruction needs
// wait states after the VALU write of its operands and before a VALU read of its results (without the s_nops the upper
// lanes read stale values).
__device__ __forceinline__ f32x2 mm_permlane32_swap(float a, float b) {
  asm volatile("s_nop 3\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 3" : "+v"(a), "+v"(b));
  return f32x2{a, b};
}

__device__ __forceinline__ float mm_xor32_sum(float x) {  // x + (x of lane ^ 32)
  const f32x2 s = mm_permlane32_swap(x, x);
  return s[0] + s[1];
}

__device__ __forceinline__ float mm_sum32(const f32x16& a, const f32x16& b) {  // sum of the lane's 32 values
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) s += a[e];
#pragma unroll
  for (int e = 0; e < 16; ++e) s += b[e];
  return s;
}

__device__ __forceinline__ float mm_m2_32(const f32x16& a, const f32x16& b, float mu) {  // sum of (v - mu)^2
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const float d = a[e] - mu;
    s = fmaf(d, d, s);
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const float d = b[e] - mu;
    s = fmaf(d, d, s);
  }
  return s;
}

__device__ __forceinline__ float mm_relu_sum32(const f32x16& a, const f32x16& b, float m1, float m0) {
  float s = 0.f;  // sum of relu(v * m1 + m0)
#pragma unroll
  for (int e = 0; e < 16; ++e) s += fmaxf(fmaf(a[e], m1, m0), 0.f);
#pragma unroll
  for (int e = 0; e < 16; ++e) s += fmaxf(fmaf(b[e], m1, m0), 0.f);
  return s;
}

// Largest magnitude handed to the fp16 `hi` half of an hl16 split (fp16 overflows to inf above 65504).
#define MM_F16_CLAMP 65000.f

// Prologue value of the normalise + ReLU kernels: relu(x * s + h), clamped to the fp16 range.  Zeroing rows past a
// tile's end and the hi / lo split (mm_split2) are the caller's.
__device__ __forceinline__ float mm_norm_relu(float x, float s, float h) {
  return fminf(fmaxf(fmaf(x, s, h), 0.f), MM_F16_CLAMP);
}

// lo half of the hl16 split of one value, given its hi half (f16)y: (f16)(y - (float)hi) - convert back, subtract, convert
// (mm_split_lo2 below: the same halves of two values with v_fma_mix).  Clamps and ReLU are the caller's.
__device__ __forceinline__ _Float16 mm_hl_lo(float y, _Float16 hi) { return (_Float16)(y - (float)hi); }

// hl16 join: the fp32 value of a (hi, lo) pair
__device__ __forceinline__ float mm_hl_join(_Float16 hi, _Float16 lo) { return (float)hi + (float)lo; }

// The lo halves of the two-term fp16 split of (y0, y1), given their rounded hi halves packed in one register:
// (f16)(y - (float)hi) per element.  v_fma_mix{lo,hi}_f16 computes an fp32 fma of mixed fp16 / fp32 sources and rounds the
// result to f16 into one half of the destination: ONE instruction per element where convert-back + subtract + convert take
// 2.5 (y - hi is exact in fp32, the rounding to f16 is the mode's RNE with subnormals kept, like v_cvt_f16_f32: bit for bit
// the three-instruction form - tests/test_gemm_f16_gpu.py compares a kernel that uses this against one that does not).
__device__ __forceinline__ unsigned mm_split_lo2(unsigned hi2, float y0, float y1) {
  unsigned lo2;
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
      : "=&v"(lo2)
      : "v"(hi2), "v"(y0), "v"(y1));
  return lo2;
}

// two values -> their packed fp16 hi halves and lo halves (RNE both; three instructions: v_cvt_pk_f16_f32 + the two above)
__device__ __forceinline__ void mm_split2(float y0, float y1, unsigned& hi2, unsigned& lo2) {
  const f16x2 h = {(_Float16)y0, (_Float16)y1};
  hi2 = __builtin_bit_cast(unsigned, h);
  lo2 = mm_split_lo2(hi2, y0, y1);
}

__device__ __forceinline__ float mm_act(float v, int act) {
  if (act == MMMOT_ACT_RELU) return fmaxf(v, 0.f);
  if (act == MMMOT_ACT_SIGMOID) return 1.f / (1.f + expf(-v));
  return v;
}

__device__ __forceinline__ float mm_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// Power-of-two scale exponent that puts amax = f * 2^ex (f in [0.5, 1)) at 2^target: target - ex, for the fp16-split
// operands of the training step (device-side scales: gradients of 1e-4 .. 1e-7, freshly updated weights).  Guarded
// (ADVICE r4): a zero, denormal-tiny, infinite or NaN amax must not turn into 2^(+-huge) = inf and 0 * inf = NaN in the
// products - a non-finite or non-positive amax means "unscaled", and the exponent is clamped to [-100, 100] (2^100 times
// a denormal is still finite; the inverse scale 2^-shift stays a normal float).
__device__ __forceinline__ int mm_pow2_shift(float amax, int target) {
  if (!(amax > 0.f) || !(amax <= 3.4028234e38f)) return 0;
  int ex = 0;
  (void)frexpf(amax, &ex);
  const int s = target - ex;
  return s < -100 ? -100 : (s > 100 ? 100 : s);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
