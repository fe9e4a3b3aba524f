// Association of a chain of T >= 2 frames (reference solvers.py:9-138, ortools_solve with any len(det_split)) as a
// min-cost flow on a layered network, solved exactly: one workgroup per chain, successive shortest augmenting paths with
// fp64 node potentials, the residual nodes spread over the lanes.
//
// Network (include/mmmot_hip.h, mmmot_associate_chains): detection v of the L = sum n_t detections has the nodes
// in(v) = v and out(v) = L + v; the sink is node 2L and the source is implicit (distance 0, scanned first).  Edges, each
// of capacity 1: source -> in(v) at -new_v, in(v) -> out(v) at -det_v, out(t, j) -> in(t + 1, k) at -link_t[j][k],
// out(v) -> sink at -end_v.  A unit of flow is a trajectory; every node carries at most one unit, so the flow is the three
// per-detection values `used`, `pred` and `succ`.  Residual edges back into the source and out of the sink never lie on a
// shortest source-sink path and are left out.
//
// The initial potentials are the shortest distances of the empty network, a DAG: one forward pass over the layers, a min
// over the previous layer with the lanes over the columns.  Per augmentation a Dijkstra runs over the 2L + 1 nodes on
// reduced costs: each step relaxes the residual edges of the newest scanned node into the lanes' unscanned nodes, then an
// arg-min (smallest node index on ties) by a wave butterfly and, with four waves, one LDS exchange and one barrier.  The
// search ends when the sink is scanned; the potentials rise by min(dist, dist of the sink); the augmentation stops at the
// first path whose true cost is >= 0 (the cost of the flow is convex in its value).  Every per-node value is computed by
// the same expression whichever lane holds it, so the one-wave and the four-wave kernel return the same bits.
#include "common.h"

#define AC_MAXT MMMOT_CHAIN_MAXT
#define AC_MAXN 512
#define AC_MAXL 1024
#define AC_ROW MMMOT_CHAIN_ROW  // ints per chain in the table: T, score offset, link offset, n_0 .. n_7

namespace {

int g_chain_variant = 0;  // 0 = automatic; see mmmot_set_chain_variant

// cost of using the variable with score s: -s, clamped so that no sum of the search can overflow; NaN: edge absent
__device__ __forceinline__ double ac_cost(float s) {
  return s == s ? -(double)fmaxf(fminf(s, 1e30f), -1e30f) : (double)INFINITY;
}

__device__ __forceinline__ void ac_better(double& bv, int& bj, double ov, int oj) {
  if (ov < bv || (ov == bv && oj < bj)) {
    bv = ov;
    bj = oj;
  }
}

// LDS layout for a launch whose chains have L <= cap (8-byte arrays first)
struct AcLds {
  double *dist, *pot, *red_v;
  int *parent, *pred, *succ, *red_j, *st, *loff;
  float *sdet, *snew, *send;
  unsigned char *used, *scanned;
  __device__ AcLds(unsigned char* base, int cap) {
    const int nn = 2 * cap + 1;
    double* d = (double*)base;
    dist = d; pot = d + nn; red_v = d + 2 * nn;
    int* q = (int*)(red_v + 8);
    parent = q; pred = q + nn; succ = q + nn + cap; red_j = q + nn + 2 * cap; st = red_j + 8; loff = st + AC_MAXT + 1;
    float* f = (float*)(loff + AC_MAXT);
    sdet = f; snew = f + cap; send = f + 2 * cap;
    used = (unsigned char*)(f + 3 * cap);
    scanned = used + cap;
  }
};

}  // namespace

static size_t ac_lds_bytes(int cap) {
  const size_t nn = 2 * (size_t)cap + 1;
  return (2 * nn + 8) * 8 + (nn + 2 * cap + 8 + AC_MAXT + 1 + AC_MAXT) * 4 + (size_t)3 * cap * 4 + cap + nn;
}

// NW waves per workgroup
template <int NW>
__global__ __launch_bounds__(64 * NW) void associate_chain_kernel(
    const float* __restrict__ det, const float* __restrict__ nsc, const float* __restrict__ esc,
    const float* __restrict__ link, const int* __restrict__ chains, int max_n, int cap, float* __restrict__ out,
    const int* __restrict__ out_off, double* __restrict__ objective) {
  constexpr int TH = 64 * NW;
  extern __shared__ __attribute__((aligned(16))) unsigned char ac_lds[];
  AcLds s(ac_lds, cap);
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int* ch = chains + AC_ROW * p;
  const int T = ch[0], so = ch[1], lo = ch[2];
  bool ok = T >= 2 && T <= AC_MAXT && so >= 0 && lo >= 0;
  int L = 0;
  if (ok) {
    for (int t = 0; t < T; ++t) {
      const int n = ch[3 + t];
      ok = ok && n >= 0 && n <= max_n && n <= AC_MAXN;
      L += ok ? n : 0;
    }
  }
  if (!ok || L < 1 || L > cap) {  // outside the launch's contract: nothing but a NaN objective is written
    if (tid == 0) objective[p] = __builtin_nan("");
    return;
  }
  const float* lk = link + lo;
  const int NN = 2 * L + 1, SINK = 2 * L;

  if (tid == 0) {  // frame starts and the offsets of the link blocks
    int a = 0, b = 0;
    for (int t = 0; t < T; ++t) {
      s.st[t] = a;
      if (t < T - 1) s.loff[t] = b;
      if (t < T - 1) b += ch[3 + t] * ch[4 + t];
      a += ch[3 + t];
    }
    s.st[T] = a;
  }
  for (int v = tid; v < L; v += TH) {
    s.sdet[v] = det[so + v];
    s.snew[v] = nsc[so + v];
    s.send[v] = esc[so + v];
    s.used[v] = 0;
    s.pred[v] = -1;
    s.succ[v] = -1;
  }
  __syncthreads();

  // initial potentials: shortest distances from the source in the empty network, layer by layer
  for (int t = 0; t < T; ++t) {
    const int a = s.st[t], n = s.st[t + 1] - a;
    const int pa = t > 0 ? s.st[t - 1] : 0, pn = t > 0 ? a - pa : 0;
    const float* blk = t > 0 ? lk + s.loff[t - 1] : lk;
    for (int k = tid; k < n; k += TH) {
      double best = ac_cost(s.snew[a + k]);
      for (int j = 0; j < pn; ++j) {
        const double cand = s.pot[L + pa + j] + ac_cost(blk[j * n + k]);
        if (cand < best) best = cand;
      }
      s.pot[a + k] = best;
      s.pot[L + a + k] = best + ac_cost(s.sdet[a + k]);
    }
    __syncthreads();
  }
  if (wv == 0) {
    double m = INFINITY;
    for (int v = lane; v < L; v += 64) m = fmin(m, s.pot[L + v] + ac_cost(s.send[v]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmin(m, __shfl_xor(m, o));
    if (lane == 0) s.pot[SINK] = m;
  }
  __syncthreads();
  double pot_sink = s.pot[SINK];  // every thread keeps the sink's potential: the true cost of the next shortest path

  int step = 0;
  for (int aug = 0; aug < L && pot_sink < 0.0; ++aug) {
    // the source's edges: into in(v) unless v already starts a trajectory
    for (int w = tid; w < NN; w += TH) {
      double d = INFINITY;
      if (w < L) {
        const double c = ac_cost(s.snew[w]), pw = s.pot[w];
        if (c < INFINITY && pw < INFINITY && !(s.used[w] && s.pred[w] < 0)) d = fmax(0.0, c - pw);
      }
      s.dist[w] = d;
      s.parent[w] = -1;
      s.scanned[w] = 0;
    }
    int u = -1;  // the newest scanned node; -1: the source
    double du = 0.0;
    bool reached = false;
    for (int it = 0; it <= NN; ++it) {
      // the residual edges of u: one single target w1 at c1, the in-nodes [ra, rb) of the next frame at the link row
      // `row` (but `skip`, the saturated link), and the sink at c_sink
      double pu = 0.0, c1 = INFINITY, c_sink = INFINITY;
      int w1 = -1, ra = 0, rb = 0, skip = -1;
      const float* row = lk;
      if (u >= 0) {
        pu = s.pot[u];
        const int v = u < L ? u : u - L;
        int t = 0;
        while (t + 1 < T && v >= s.st[t + 1]) ++t;
        const bool usedv = s.used[v] != 0;
        if (u < L) {
          if (!usedv) {  // in(v) -> out(v)
            w1 = L + v;
            c1 = ac_cost(s.sdet[v]);
          } else if (s.pred[v] >= 0) {  // the link pred -> v undone: in(v) -> out(pred)
            const int pv = s.pred[v];
            w1 = L + pv;
            c1 = -ac_cost(lk[s.loff[t - 1] + (pv - s.st[t - 1]) * (s.st[t + 1] - s.st[t]) + (v - s.st[t])]);
          }
        } else {
          if (t < T - 1) {
            ra = s.st[t + 1];
            rb = s.st[t + 2];
            row = lk + s.loff[t] + (v - s.st[t]) * (rb - ra);
          }
          const int sv = usedv ? s.succ[v] : -2;
          skip = sv;
          if (sv != -1) c_sink = ac_cost(s.send[v]);
          if (usedv) {  // detection v dropped: out(v) -> in(v)
            w1 = v;
            c1 = -ac_cost(s.sdet[v]);
          }
        }
      }
      double bv = INFINITY;
      int bj = 0x7fffffff;
      for (int w = tid; w < NN; w += TH) {
        if (!s.scanned[w]) {
          double d = s.dist[w];
          double c = INFINITY;
          if (w == w1) c = c1;
          else if (w >= ra && w < rb) c = w != skip ? ac_cost(row[w - ra]) : (double)INFINITY;
          else if (w == SINK) c = c_sink;
          const double pw = s.pot[w];
          if (c < INFINITY && pw < INFINITY) {
            const double nd = du + fmax(0.0, (c + pu) - pw);
            if (nd < d) {
              d = nd;
              s.dist[w] = nd;
              s.parent[w] = u;
            }
          }
          if (d < bv) {  // w ascending: strict < keeps the smallest index
            bv = d;
            bj = w;
          }
        }
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) ac_better(bv, bj, __shfl_xor(bv, o), __shfl_xor(bj, o));
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
        for (int w = 1; w < NW; ++w) ac_better(bv, bj, s.red_v[par + w], s.red_j[par + w]);
      }
      ++step;
      if (!(bv < INFINITY)) break;  // the sink cannot be reached any more
      u = bj;
      du = bv;
      if (u % TH == tid) s.scanned[u] = 1;
      if (u == SINK) {
        reached = true;
        break;
      }
    }
    if (!reached || !(pot_sink + du < 0.0)) break;  // no path, or the cheapest one gains nothing: the flow is optimal
    pot_sink += du;
    for (int w = tid; w < NN; w += TH) {
      const double pw = s.pot[w];
      if (pw < INFINITY) s.pot[w] = pw + fmin(s.dist[w], du);
    }
    __syncthreads();
    if (tid == 0) {  // augment along the parents: every field is set by exactly one edge of the (simple) path
      int w = SINK;
      for (int guard = 0; guard <= NN; ++guard) {
        const int q = s.parent[w];
        if (q < 0) {  // source -> in(w)
          s.pred[w] = -1;
          break;
        }
        if (w == SINK) s.succ[q - L] = -1;       // out(v) -> sink
        else if (w >= L && q == w - L) s.used[q] = 1;  // in(v) -> out(v)
        else if (w < L && q == w + L) {          // out(v) -> in(v): v leaves its trajectory
          s.used[w] = 0;
          s.pred[w] = -1;
          s.succ[w] = -1;
        } else if (w < L) {                      // out(a) -> in(w): a new link
          s.pred[w] = q - L;
          s.succ[q - L] = w;
        }                                        // in(k) -> out(v), an undone link: both ends are set by their other edges
        w = q;
      }
    }
    __syncthreads();
  }

  // ortools-shaped results: [det L | new L | end L | link_0 | .. | link_{T-2}], written once each with plain stores
  float* o = out + out_off[p];
  for (int v = tid; v < L; v += TH) {
    const bool us = s.used[v] != 0;
    o[v] = us ? 1.f : 0.f;
    o[L + v] = us && s.pred[v] < 0 ? 1.f : 0.f;
    o[2 * L + v] = us && s.succ[v] < 0 ? 1.f : 0.f;
  }
  for (int t = 0; t < T - 1; ++t) {
    const int a = s.st[t], b = s.st[t + 1], n1 = s.st[t + 2] - b;
    float* ol = o + 3 * L + s.loff[t];
    for (int e = tid; e < (b - a) * n1; e += TH) {
      const int i = e / n1, k = e - i * n1;
      ol[e] = s.used[a + i] && s.succ[a + i] == b + k ? 1.f : 0.f;
    }
  }
  // objective: wave 0 only (the same sums whatever NW), lane-strided partials then a butterfly
  if (wv == 0) {
    double acc = 0.0;
    for (int v = lane; v < L; v += 64) {
      if (s.used[v]) {
        double x = (double)s.sdet[v];
        if (s.pred[v] < 0) x += (double)s.snew[v];
        const int sv = s.succ[v];
        if (sv < 0) {
          x += (double)s.send[v];
        } else {
          int t = 0;
          while (t + 1 < T && v >= s.st[t + 1]) ++t;
          x += (double)lk[s.loff[t] + (v - s.st[t]) * (s.st[t + 2] - s.st[t + 1]) + (sv - s.st[t + 1])];
        }
        acc += x;
      }
    }
#pragma unroll
    for (int o2 = 32; o2 >= 1; o2 >>= 1) acc += __shfl_xor(acc, o2);
    if (lane == 0) objective[p] = acc;
  }
}

template <int NW>
static int ac_launch(const float* det, const float* nsc, const float* esc, const float* link, const int* chains, int B,
                     int max_n, int cap, float* out, const int* out_off, double* objective, hipStream_t st) {
  const size_t lds = ac_lds_bytes(cap);  // 64697 bytes at cap = 1024: within the 64 KB a kernel gets without asking
  if (lds > 64 * 1024) return MMMOT_EINVAL;
  hipLaunchKernelGGL(associate_chain_kernel<NW>, dim3(B), dim3(64 * NW), lds, st, det, nsc, esc, link, chains, max_n,
                     cap, out, out_off, objective);
  return mm_check(hipGetLastError());
}

extern "C" int mmmot_set_chain_variant(int v) {
  if (v < 0 || v > 2) return MMMOT_EINVAL;
  g_chain_variant = v;
  return MMMOT_OK;
}

extern "C" int mmmot_associate_chains(const float* det, const float* new_score, const float* end_score,
                                      const float* link, const int* chains, int B, int max_n, int max_L, float* out,
                                      const int* out_off, double* objective, void* stream) {
  if (!det || !new_score || !end_score || !link || !chains || !out || !out_off || !objective) return MMMOT_EINVAL;
  if (B < 1 || max_n < 1 || max_n > AC_MAXN || max_L < 1 || max_L > AC_MAXL || max_n > max_L) return MMMOT_EINVAL;
  if ((long)max_L > (long)AC_MAXT * max_n) return MMMOT_EINVAL;  // at most 8 frames of at most max_n each
  int var = g_chain_variant;
  if (var == 0) var = 2 * max_L + 1 <= 256 ? 1 : 2;
  hipStream_t st = (hipStream_t)stream;
  if (var == 1)
    return ac_launch<1>(det, new_score, end_score, link, chains, B, max_n, max_L, out, out_off, objective, st);
  return ac_launch<4>(det, new_score, end_score, link, chains, B, max_n, max_L, out, out_off, objective, st);
}
