// One-launch Adam step over every tensor of an optimizer (include/mmmot_hip.h: mmmot_adam_step, mmmot_adam_chunks,
// mmmot_adam_chunk_elems).
//
// Multi-tensor apply: a device table holds one 64-byte row per tensor (the four base pointers, numel, the per-tensor
// scalars of this step, flags), a device chunk table one (tensor index, chunk index) row per MMMOT_ADAM_CHUNK elements of
// a tensor.  One workgroup of 256 threads serves one chunk: it reads p, g, m, v once and writes p, m, v once - 28 bytes an
// element, the least an Adam step can move.  No LDS, no atomics, no reduction: every element is read and written by
// exactly one lane, so the result depends neither on the chunk geometry nor on the order of the tables.
//
// The arithmetic is torch's single-tensor Adam in fp32, one IEEE operation per step: no contraction into FMAs in this
// file.  Division and square root are the correctly rounded ones (hipcc's default for fp32).
#pragma clang fp contract(off)
#include "common.h"

#define AD_THREADS 256
#define AD_CHUNK MMMOT_ADAM_CHUNK
#define AD_VECS (AD_CHUNK / (4 * AD_THREADS))  // 16-byte groups per lane and array: 4
#define AD_SCALARS (AD_CHUNK / AD_THREADS)     // elements per lane on the scalar path: 16, taken four at a time

static_assert(sizeof(mmmot_adam_row) == 64, "mmmot_adam_row is 64 bytes (mmmot_amd/torch_ops.py packs it)");
static_assert(AD_CHUNK % (4 * AD_THREADS) == 0 && AD_SCALARS % 4 == 0, "a chunk is whole 16-byte groups per lane");

// the table's pointers are global memory: said so, the accesses are global_load / global_store, not flat ones (a flat
// access counts on both wait counters and the compiler then drains both)
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) const float gcfloat;
typedef __attribute__((address_space(1))) f32x4 gvec;
typedef __attribute__((address_space(1))) const f32x4 gcvec;

struct AdamConsts {
  float omb1, b2, omb2, eps;  // 1 - beta1, beta2, 1 - beta2 (the differences taken in double, rounded once), eps
};

__device__ __forceinline__ void ad_elem(float& p, float g, float& m, float& v, float step_size, float bc2_sqrt, float decay,
                                        float l2, const AdamConsts& k) {
  if (decay != 1.f) p = p * decay;
  if (l2 != 0.f) g = g + l2 * p;
  m = m + k.omb1 * (g - m);
  v = v * k.b2 + k.omb2 * g * g;
  const float denom = sqrtf(v) / bc2_sqrt + k.eps;
  p = p - step_size * (m / denom);
}

// n elements (1 <= n <= AD_CHUNK) of one tensor; FULL: n == AD_CHUNK, no lane is masked
template <bool FULL>
__device__ __forceinline__ void ad_chunk_vec(gfloat* __restrict__ p, gcfloat* __restrict__ g, gfloat* __restrict__ m,
                                             gfloat* __restrict__ v, int n, int tid, float step_size, float bc2_sqrt,
                                             float decay, float l2, const AdamConsts& k) {
  const int nv = n >> 2;  // whole 16-byte groups; the 0 .. 3 elements behind them go one to a lane
  f32x4 P[AD_VECS], G[AD_VECS], M[AD_VECS], V[AD_VECS];
#pragma unroll
  for (int j = 0; j < AD_VECS; ++j) {
    const int i = j * AD_THREADS + tid;
    if (FULL || i < nv) {
      P[j] = reinterpret_cast<gvec*>(p)[i];
      G[j] = reinterpret_cast<gcvec*>(g)[i];
      M[j] = reinterpret_cast<gvec*>(m)[i];
      V[j] = reinterpret_cast<gvec*>(v)[i];
    }
  }
  const int t = 4 * nv + tid;
  const bool tail = !FULL && tid < 4 && t < n;
  float tp = 0.f, tg = 0.f, tm = 0.f, tv = 0.f;
  if (tail) {
    tp = p[t];
    tg = g[t];
    tm = m[t];
    tv = v[t];
  }
#pragma unroll
  for (int j = 0; j < AD_VECS; ++j) {
    const int i = j * AD_THREADS + tid;
    if (FULL || i < nv) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = P[j][e], me = M[j][e], ve = V[j][e];
        ad_elem(pe, G[j][e], me, ve, step_size, bc2_sqrt, decay, l2, k);
        P[j][e] = pe;
        M[j][e] = me;
        V[j][e] = ve;
      }
      reinterpret_cast<gvec*>(p)[i] = P[j];
      reinterpret_cast<gvec*>(m)[i] = M[j];
      reinterpret_cast<gvec*>(v)[i] = V[j];
    }
  }
  if (tail) {
    ad_elem(tp, tg, tm, tv, step_size, bc2_sqrt, decay, l2, k);
    p[t] = tp;
    m[t] = tm;
    v[t] = tv;
  }
}

// the same for bases that are only 4-byte aligned: one element per load, four of a lane's sixteen at a time
__device__ __forceinline__ void ad_chunk_scalar(gfloat* __restrict__ p, gcfloat* __restrict__ g, gfloat* __restrict__ m,
                                                gfloat* __restrict__ v, int n, int tid, float step_size, float bc2_sqrt,
                                                float decay, float l2, const AdamConsts& k) {
  for (int b = 0; b < AD_SCALARS; b += 4) {
    if (b * AD_THREADS >= n) break;  // uniform
    float P[4], G[4], M[4], V[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = (b + j) * AD_THREADS + tid;
      if (i < n) {
        P[j] = p[i];
        G[j] = g[i];
        M[j] = m[i];
        V[j] = v[i];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = (b + j) * AD_THREADS + tid;
      if (i < n) {
        ad_elem(P[j], G[j], M[j], V[j], step_size, bc2_sqrt, decay, l2, k);
        p[i] = P[j];
        m[i] = M[j];
        v[i] = V[j];
      }
    }
  }
}

// a tensor without a gradient: p = p * decay and nothing else (the caller left out decay == 1)
__device__ __forceinline__ void ad_chunk_decay(gfloat* __restrict__ p, int n, int tid, float decay, bool al) {
  if (al) {
    const int nv = n >> 2;
    f32x4 P[AD_VECS];
#pragma unroll
    for (int j = 0; j < AD_VECS; ++j) {
      const int i = j * AD_THREADS + tid;
      if (i < nv) P[j] = reinterpret_cast<gvec*>(p)[i];
    }
#pragma unroll
    for (int j = 0; j < AD_VECS; ++j) {
      const int i = j * AD_THREADS + tid;
      if (i < nv) {
#pragma unroll
        for (int e = 0; e < 4; ++e) P[j][e] = P[j][e] * decay;
        reinterpret_cast<gvec*>(p)[i] = P[j];
      }
    }
    const int t = 4 * nv + tid;
    if (tid < 4 && t < n) p[t] = p[t] * decay;
  } else {
    for (int i = tid; i < n; i += AD_THREADS) p[i] = p[i] * decay;
  }
}

__global__ __launch_bounds__(AD_THREADS) void adam_step_kernel(const mmmot_adam_row* __restrict__ table, int n_tensors,
                                                                const int* __restrict__ chunks, AdamConsts k) {
  const int tid = threadIdx.x;
  const int ti = chunks[2 * blockIdx.x], ci = chunks[2 * blockIdx.x + 1];
  if (ti < 0 || ti >= n_tensors || ci < 0) return;  // a row outside the tensor table: nothing of it is touched
  const mmmot_adam_row r = table[ti];               // wave-uniform
  const long long off = (long long)ci * AD_CHUNK;
  if (off >= r.numel) return;
  const bool has_grad = (r.flags & MMMOT_ADAM_HAS_GRAD) != 0;
  if (!has_grad && r.decay == 1.f) return;
  const long long left = r.numel - off;
  const int n = left < AD_CHUNK ? (int)left : AD_CHUNK;
  gfloat* p = (gfloat*)r.p + off;  // off is a multiple of 4096 elements: the chunk is aligned as the base is
  if (!has_grad) {
    ad_chunk_decay(p, n, tid, r.decay, (((uintptr_t)r.p) & 15u) == 0);
    return;
  }
  gcfloat* g = (gcfloat*)r.g + off;
  gfloat* m = (gfloat*)r.m + off;
  gfloat* v = (gfloat*)r.v + off;
  const bool al = ((((uintptr_t)r.p) | ((uintptr_t)r.g) | ((uintptr_t)r.m) | ((uintptr_t)r.v)) & 15u) == 0;
  if (!al)
    ad_chunk_scalar(p, g, m, v, n, tid, r.step_size, r.bc2_sqrt, r.decay, r.l2, k);
  else if (n == AD_CHUNK)
    ad_chunk_vec<true>(p, g, m, v, n, tid, r.step_size, r.bc2_sqrt, r.decay, r.l2, k);
  else
    ad_chunk_vec<false>(p, g, m, v, n, tid, r.step_size, r.bc2_sqrt, r.decay, r.l2, k);
}

extern "C" int mmmot_adam_chunk_elems(void) { return AD_CHUNK; }

extern "C" int mmmot_adam_chunks(const long long* h_numel, int n_tensors, int* h_chunks, long long cap,
                                 long long* h_count) {
  if (!h_numel || !h_count || n_tensors < 1 || cap < 0 || (cap > 0 && !h_chunks)) return MMMOT_EINVAL;
  long long total = 0;
  for (int t = 0; t < n_tensors; ++t) {
    const long long n = h_numel[t];
    if (n < 1) return MMMOT_EINVAL;
    const long long c = (n - 1) / AD_CHUNK + 1;  // no overflow for any n >= 1
    if (c > 0x7fffffffLL || total + c > 0x7fffffffLL) return MMMOT_EINVAL;  // chunk indices and the grid are 32-bit
    total += c;
  }
  *h_count = total;
  if (!h_chunks) return MMMOT_OK;  // the count alone
  if (cap < total) return MMMOT_EINVAL;
  long long w = 0;
  for (int t = 0; t < n_tensors; ++t) {
    const long long c = (h_numel[t] - 1) / AD_CHUNK + 1;
    for (long long i = 0; i < c; ++i, ++w) {
      h_chunks[2 * w] = t;
      h_chunks[2 * w + 1] = (int)i;
    }
  }
  return MMMOT_OK;
}

extern "C" int mmmot_adam_step(const mmmot_adam_row* table, int n_tensors, const int* chunks, int n_chunks, double beta1,
                               double beta2, double eps, void* stream) {
  if (!table || !chunks) return MMMOT_EINVAL;
  if (n_tensors < 1 || n_chunks < 1) return MMMOT_EINVAL;
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return MMMOT_EINVAL;  // NaN fails both
  if (!(eps >= 0.0) || !(eps <= 3.4028234e38)) return MMMOT_EINVAL;
  if ((((uintptr_t)table) & 7u) || (((uintptr_t)chunks) & 3u)) return MMMOT_EINVAL;
  AdamConsts k;
  k.omb1 = (float)(1.0 - beta1);
  k.b2 = (float)beta2;
  k.omb2 = (float)(1.0 - beta2);
  k.eps = (float)eps;
  hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)n_chunks), dim3(AD_THREADS), 0, (hipStream_t)stream, table,
                     n_tensors, chunks, k);
  return mm_check(hipGetLastError());
}
