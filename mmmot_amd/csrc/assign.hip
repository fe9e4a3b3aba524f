// Frame-pair association (reference solvers.py ortools_solve with two frames) as a maximum-weight bipartite matching,
// solved exactly: one workgroup per pair, a shortest-augmenting-path assignment (Hungarian / Jonker-Volgenant) with
// fp64 dual potentials, columns spread over the lanes.
//
// Reduction (include/mmmot_hip.h, mmmot_associate_pairs): with a_i = det_i + new_i, ua_i = max(0, a_i + end_i) for the
// N detections of frame 0 and b_j = det_{N+j} + end_{N+j}, vb_j = max(0, b_j + new_{N+j}) for the M of frame 1, the
// gain of linking i -> j is g_ij = link_ij + (a_i - ua_i) + (b_j - vb_j) and the optimum of the binary program is
// sum ua + sum vb + max over matchings of sum max(g_ij, 0).  The solver assigns every one of R = min(N, M) rows to one
// of C = max(N, M) columns (rows are frame 1 when N > M: transposed) at cost -max(g, 0); pairs with g <= 0 are then
// dropped, which is the same optimum.
//
// Per row the Dijkstra search runs over the columns: each step is a relax of the lane's unscanned columns against the
// newest tree row, then an arg-min (smallest column index on ties) by a wave butterfly and, with four waves, one LDS
// exchange and one barrier.  The duals are updated once per row at the end of its search (shortest-path form), so the
// potentials the steps read are constant during a search.  Every per-column value is computed by the same expression
// whichever lane holds it, so the one-wave and four-wave kernels and the LDS-staged variants return the same bits.
#include "common.h"

#define AS_MAXN 512

namespace {

int g_assign_variant = 0;  // 0 = automatic; see mmmot_set_assign_variant

// the gain of linking frame-0 detection i to frame-1 detection j, one fixed evaluation order everywhere
__device__ __forceinline__ double as_gain(float l, double t0, double t1) { return ((double)l + t0) + t1; }

// cost of an assignment edge: -max(g, 0), gains clamped so that no sum of the search can overflow (NaN: no gain)
__device__ __forceinline__ double as_cost(double g) { return g > 0.0 ? -fmin(g, 1e30) : 0.0; }

__device__ __forceinline__ void as_better(double& bv, int& bj, double ov, int oj) {
  if (ov < bv || (ov == bv && oj < bj)) {
    bv = ov;
    bj = oj;
  }
}

// LDS layout for a launch whose pairs have N, M <= cap (8-byte arrays first)
struct AsLds {
  double *u, *t0, *t1, *ua, *vb, *gm, *red_v;
  int *row4col, *col4row, *path, *m0, *m1, *red_j;
  float* stage;
  __device__ AsLds(unsigned char* base, int cap) {
    double* d = (double*)base;
    u = d; t0 = d + cap; t1 = d + 2 * cap; ua = d + 3 * cap; vb = d + 4 * cap; gm = d + 5 * cap; red_v = d + 6 * cap;
    int* q = (int*)(red_v + 8);
    row4col = q; col4row = q + cap; path = q + 2 * cap; m0 = q + 3 * cap; m1 = q + 4 * cap; red_j = q + 5 * cap;
    stage = (float*)(red_j + 8);
  }
};

}  // namespace

static size_t as_lds_bytes(int cap, bool stage) {
  return (size_t)(6 * cap + 8) * 8 + (size_t)(5 * cap + 8) * 4 + (stage ? (size_t)cap * cap * 4 : 0);
}

// NW waves per workgroup; STAGE: the pair's link block is copied into LDS (in the solve's row-major orientation) first
template <int NW, bool STAGE>
__global__ __launch_bounds__(64 * NW) void associate_kernel(
    const float* __restrict__ det, const float* __restrict__ nsc, const float* __restrict__ esc,
    const float* __restrict__ link, const int* __restrict__ pairs, int cap, float* __restrict__ out,
    const int* __restrict__ out_off, double* __restrict__ objective) {
  constexpr int T = 64 * NW, K = AS_MAXN / T;
  extern __shared__ __attribute__((aligned(16))) unsigned char as_lds[];
  AsLds s(as_lds, cap);
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int N = pairs[4 * p], M = pairs[4 * p + 1], so = pairs[4 * p + 2], lo = pairs[4 * p + 3];
  if (N < 1 || M < 1 || N > cap || M > cap) {  // outside the launch's contract: nothing but a NaN objective is written
    if (tid == 0) objective[p] = __builtin_nan("");
    return;
  }
  const float* dt = det + so;
  const float* nw = nsc + so;
  const float* en = esc + so;
  const float* lk = link + lo;
  const bool tr = N > M;
  const int R = tr ? M : N, C = tr ? N : M, L = N + M;

  // per-detection terms of the gain and the values of the unmatched detections (fp64 from the fp32 scores)
  for (int i = tid; i < N; i += T) {
    const double a = (double)dt[i] + (double)nw[i];
    const double ua = fmax(0.0, a + (double)en[i]);
    s.t0[i] = a - ua;
    s.ua[i] = ua;
    s.m0[i] = -1;
  }
  for (int j = tid; j < M; j += T) {
    const double b = (double)dt[N + j] + (double)en[N + j];
    const double vb = fmax(0.0, b + (double)nw[N + j]);
    s.t1[j] = b - vb;
    s.vb[j] = vb;
    s.m1[j] = -1;
  }
  for (int r = tid; r < R; r += T) {
    s.u[r] = 0.0;
    s.col4row[r] = -1;
  }
  for (int j = tid; j < C; j += T) {
    s.row4col[j] = -1;
    s.path[j] = -1;
  }
  if (STAGE) {
    for (int e = tid; e < R * C; e += T) {
      const int r = e / C, c = e - r * C;
      s.stage[e] = tr ? lk[c * M + r] : lk[r * M + c];
    }
  }
  __syncthreads();
  const double* rterm = tr ? s.t1 : s.t0;
  const double* cterm = tr ? s.t0 : s.t1;
  double v[K], ct[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int j = k * T + tid;
    v[k] = 0.0;
    ct[k] = j < C ? cterm[j] : 0.0;
  }

  int step = 0;
  for (int cur = 0; cur < R; ++cur) {
    double sp[K];
#pragma unroll
    for (int k = 0; k < K; ++k) sp[k] = INFINITY;
    unsigned scanned = 0;  // bit k: this lane's column k * T + tid is in the search tree
    double minv = 0.0;
    int i = cur, sink = -1;
    for (;;) {
      const double ui = s.u[i], rti = rterm[i];
      double bv = INFINITY;
      int bj = 0x7fffffff;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int j = k * T + tid;
        if (j < C && !((scanned >> k) & 1u)) {
          const float l = STAGE ? s.stage[i * C + j] : (tr ? lk[j * M + i] : lk[i * M + j]);
          const double g = tr ? as_gain(l, ct[k], rti) : as_gain(l, rti, ct[k]);
          const double r = minv + as_cost(g) - ui - v[k];
          if (r < sp[k]) {
            sp[k] = r;
            s.path[j] = i;
          }
          if (sp[k] < bv) {  // k ascending: j ascending, strict < keeps the smallest index
            bv = sp[k];
            bj = j;
          }
        }
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) as_better(bv, bj, __shfl_xor(bv, o), __shfl_xor(bj, o));
      if (NW > 1) {
        const int par = (step & 1) * 4;  // two slot sets: the next step's writes cannot overtake this step's reads
        if (lane == 0) {
          s.red_v[par + wv] = bv;
          s.red_j[par + wv] = bj;
        }
        __syncthreads();
        bv = s.red_v[par];
        bj = s.red_j[par];
#pragma unroll
        for (int w = 1; w < NW; ++w) as_better(bv, bj, s.red_v[par + w], s.red_j[par + w]);
      }
      ++step;
      if (bj >= C) break;  // no finite candidate (cannot happen with finite scores): leave the row unassigned
      minv = bv;
      if (bj % T == tid) scanned |= 1u << (bj / T);
      const int nxt = s.row4col[bj];
      if (nxt < 0) {
        sink = bj;
        break;
      }
      i = nxt;
    }
    if (sink >= 0) {
      // duals of the tree: rows reached through a scanned column and the scanned columns themselves
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int j = k * T + tid;
        if ((scanned >> k) & 1u) {
          const double d = minv - sp[k];
          v[k] -= d;
          if (j != sink) s.u[s.row4col[j]] += d;
        }
      }
      if (tid == 0) s.u[cur] += minv;
    }
    __syncthreads();
    if (tid == 0 && sink >= 0) {  // augment along the predecessor chain
      int j = sink;
      for (;;) {
        const int r = s.path[j];
        s.row4col[j] = r;
        const int prev = s.col4row[r];
        s.col4row[r] = j;
        j = prev;
        if (r == cur) break;
      }
    }
    __syncthreads();
  }

  // drop the rows whose partner gains nothing; record both directions and the gains of the kept pairs
  for (int r = tid; r < R; r += T) {
    const int c = s.col4row[r];
    const int i = tr ? c : r, j = tr ? r : c;
    if (c >= 0) {
      const double g = as_gain(lk[i * M + j], s.t0[i], s.t1[j]);
      if (g > 0.0) {
        s.m0[i] = j;
        s.m1[j] = i;
        s.gm[i] = g;
      }
    }
  }
  __syncthreads();

  // ortools-shaped results: [det L | new L | end L | link N*M], written once each with plain stores
  float* o = out + out_off[p];
  for (int d = tid; d < L; d += T) {
    float vd, vn, ve;
    if (d < N) {
      const bool m = s.m0[d] >= 0;
      const float x = s.ua[d] > 0.0 ? 1.f : 0.f;
      vd = m ? 1.f : x;
      vn = m ? 1.f : x;
      ve = m ? 0.f : x;
    } else {
      const bool m = s.m1[d - N] >= 0;
      const float x = s.vb[d - N] > 0.0 ? 1.f : 0.f;
      vd = m ? 1.f : x;
      vn = m ? 0.f : x;
      ve = m ? 1.f : x;
    }
    o[d] = vd;
    o[L + d] = vn;
    o[2 * L + d] = ve;
  }
  for (int e = tid; e < N * M; e += T) {
    const int i = e / M, j = e - i * M;
    o[3 * L + e] = s.m0[i] == j ? 1.f : 0.f;
  }
  // objective: wave 0 only (the same sums whatever NW), lane-strided partials then a butterfly
  if (wv == 0) {
    double acc = 0.0;
    for (int d = lane; d < N; d += 64) acc += s.ua[d] + (s.m0[d] >= 0 ? s.gm[d] : 0.0);
    for (int d = lane; d < M; d += 64) acc += s.vb[d];
#pragma unroll
    for (int o2 = 32; o2 >= 1; o2 >>= 1) acc += __shfl_xor(acc, o2);
    if (lane == 0) objective[p] = acc;
  }
}

template <int NW, bool STAGE>
static int as_launch(const float* det, const float* nsc, const float* esc, const float* link, const int* pairs, int B,
                     int cap, float* out, const int* out_off, double* objective, hipStream_t st) {
  const size_t lds = as_lds_bytes(cap, STAGE);
  auto kern = associate_kernel<NW, STAGE>;
  if (lds > 64 * 1024) {  // the staged 128 x 128 block: raise the kernel's dynamic LDS limit once (160 KB on gfx950)
    static const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                    (int)as_lds_bytes(128, true));
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3(B), dim3(64 * NW), lds, st, det, nsc, esc, link, pairs, cap, out, out_off, objective);
  return mm_check(hipGetLastError());
}

extern "C" int mmmot_set_assign_variant(int v) {
  if (v < 0 || v > 4) return MMMOT_EINVAL;
  g_assign_variant = v;
  return MMMOT_OK;
}

extern "C" int mmmot_associate_pairs(const float* det, const float* new_score, const float* end_score,
                                     const float* link, const int* pairs, int B, int max_nm, float* out,
                                     const int* out_off, double* objective, void* stream) {
  if (!det || !new_score || !end_score || !link || !pairs || !out || !out_off || !objective) return MMMOT_EINVAL;
  if (B < 1 || max_nm < 1 || max_nm > AS_MAXN) return MMMOT_EINVAL;
  int var = g_assign_variant;
  if (var == 0) var = max_nm <= 128 ? 3 : 2;  // measured: one staged wave is fastest up to 128 x 128
  if (var >= 3 && max_nm > 128) return MMMOT_EINVAL;  // the staged link block is at most 128 x 128 fp32 (64 KB)
  hipStream_t st = (hipStream_t)stream;
  switch (var) {
    case 1: return as_launch<1, false>(det, new_score, end_score, link, pairs, B, max_nm, out, out_off, objective, st);
    case 2: return as_launch<4, false>(det, new_score, end_score, link, pairs, B, max_nm, out, out_off, objective, st);
    case 3: return as_launch<1, true>(det, new_score, end_score, link, pairs, B, max_nm, out, out_off, objective, st);
    default: return as_launch<4, true>(det, new_score, end_score, link, pairs, B, max_nm, out, out_off, objective, st);
  }
}
