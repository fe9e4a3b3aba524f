// Association of a WHOLE sequence of T frames (reference solvers.py:9-138, ortools_solve at len(det_split) = T) as one
// min-cost flow on the layered network of assign_chain.hip, for T up to 4096 and L = sum n_t up to 65536, with SKIP LINKS:
// arcs out(t, j) -> in(t + g, k) for every gap g = 1 .. G (G <= 8), so that a trajectory may miss up to G - 1 frames.
// Next-frame links are the case G = 1.  The network is layered with unit capacities: one workgroup per sequence,
// successive shortest augmenting paths, each found by a label-correcting search over the layers.
// mmmot_associate_sequences launches the kernels compiled for G = 1 (GAPS = false: every gap expression folds),
// mmmot_associate_sequences_gap those that take G at run time, also at G = 1, where they return the same bits.
//
// Network (include/mmmot_hip.h, mmmot_associate_sequences[_gap]): in(v) = v, out(v) = L + v, the sink is node 2L, the
// source is node -1.  Edges of capacity 1 at cost -score (fp64 from the fp32 scores): source -> in(v) (-new_v),
// in(v) -> out(v) (-det_v), out(t, j) -> in(t + g, k) (-link^g_t[j][k]), out(v) -> sink (-end_v).  A unit of flow is a
// trajectory; the flow is `used`, `pred` and `succ` per detection, and `inl` keeps the score of the link pred(v) -> v.
// The link blocks lie gap by gap: all g = 1 blocks in frame order, then all g = 2 blocks, ..; the offset of block (g, t)
// is loff[(g - 1) * T + t].
//
// Search.  The residual network of a minimum-cost flow has no negative cycle, so the labels are true path costs and no
// potentials are kept.  All labels start at +inf.  One PASS is
//   a forward sweep, frame 0 .. T-1: din(k) = min(din(k), -new_k, min dout(j) - link[j][k]) over the unsaturated edges
//   from the detections j of the frames t-G .. t-1 - they are the contiguous detection indices [st[t-G], st[t]), visited
//   in ascending order - then dout(k) = min(dout(k), din(k) - det_k) when k is unused;
//   a backward sweep, frame T-1 .. 0, over the used detections only (the residual back-edges run along trajectories):
//   din(k) = min(din(k), dout(k) + det_k), then dout(pred k) = min(dout(pred k), din(k) + link[pred k][k]); pred k lies
//   up to G frames back.
// After a forward sweep every forward edge is relaxed, after a backward sweep every back-edge: a backward sweep that lowers
// nothing ends the search with exact labels.  The passes number 1 + the times the shortest path turns back in time.
// A sweep visits only the frames whose inputs the sweep before it lowered, and goes on beyond them while it lowers
// something itself (the first pass of every search, from the empty labels, is full).  A frame that lowers a label
// changes the inputs of the G frames after it (forward) or before it (backward), so every range is wider by the gap: a
// forward sweep ends at the first frame that lowers nothing and lies G or more behind the last one that did; a backward
// sweep likewise; labels lowered at frame t by a backward sweep make the next forward sweep visit the frames
// t-G+1 .. t+G-1.  The ranges only ever include frames with unchanged inputs, so the result is that of full sweeps.
// Labels are NOT carried from one augmentation to the next.
// A label is lowered on a strict decrease only (the parents then form a tree); inside one minimum the smallest node index
// wins a tie, the source before every out(j) - with global detection indices the earlier frame wins.  Each value is
// formed by the same expression on whichever lane holds it, so the one-wave, the four-wave, the LDS-resident and the
// global-memory kernel return the same bits.
//
// Bounds.  Augmentations <= L, passes per augmentation <= 2L + 2, path walk <= 2L + 2 steps.  A bound that is hit ends
// the sequence with a NaN objective and a status word: no loop of this file runs on a condition alone.
#include "common.h"

#define SQ_ROW MMMOT_SEQ_ROW
#define SQ_MAXT MMMOT_SEQ_MAXT
#define SQ_MAXN 512
#define SQ_MAXL MMMOT_SEQ_MAXL
#define SQ_MAXGAP MMMOT_SEQ_MAXGAP
#define SQ_STATE_BYTES 53  // per detection: din, dout fp64; pin, pout, pred, succ int32; inl, pls, det, new, end fp32; used byte
#define SQ_LDS_CAP 2304    // the largest L whose state lives in LDS
// the largest dynamic-LDS request: frame starts and one offset row at T = 4096, and the state of 2304 detections
// (53 * 2304 = 122 112 bytes of the CU's 160 KB, beside 32 784).  The G x T offset table of more gaps sits in LDS only
// where it fits below this beside the rest.
#define SQ_LDS_BYTES (((((size_t)2 * SQ_MAXT + 2) * 4 + 15) & ~(size_t)15) + (size_t)SQ_STATE_BYTES * SQ_LDS_CAP)

namespace {

int g_seq_variant = 0;      // 0 = automatic; see mmmot_set_sequence_variant
int g_seq_gap_variant = 0;  // the same for mmmot_associate_sequences_gap; see mmmot_set_sequence_gap_variant

// cost of using the variable with score s: -s, clamped so that no sum of the search can overflow; NaN: edge absent
__device__ __forceinline__ double sq_cost(float s) {
  return s == s ? -(double)fmaxf(fminf(s, 1e30f), -1e30f) : (double)INFINITY;
}

struct SqState {
  double *din, *dout;
  int *pin, *pout, *pred, *succ;
  float *inl, *pls, *sdet, *snew, *send;  // the last three: the sequence's scores, read at every frame step
  unsigned char* used;
  __device__ SqState(unsigned char* base, int L) {
    din = (double*)base;
    dout = din + L;
    pin = (int*)(dout + L);
    pout = pin + L;
    pred = pout + L;
    succ = pred + L;
    inl = (float*)(succ + L);
    pls = inl + L;
    sdet = pls + L;
    snew = sdet + L;
    send = snew + L;
    used = (unsigned char*)(send + L);
  }
};

}  // namespace

// bytes at the head of the dynamic LDS: the frame starts [max_T + 1], then - when it lives there - the offset table
// [max_gap * max_T]
__host__ __device__ static inline size_t sq_frames_bytes(int max_T, int max_gap, bool tab_lds) {
  return (((size_t)max_T + 1 + (tab_lds ? (size_t)max_gap * max_T : 0)) * 4 + 15) & ~(size_t)15;
}

// NW waves per workgroup; LDS: the state lives in dynamic LDS (L <= SQ_LDS_CAP), else in the workspace; GAPS: the gap
// count is gp_arg and the offset table lives in LDS where tab_arg says so, else at the head of the sequence's workspace;
// without GAPS the links are next-frame ones (gap count 1, the one table row in LDS, no table room in the workspace)
template <int NW, bool LDS, bool GAPS>
__global__ __launch_bounds__(64 * NW) void associate_sequence_kernel(
    const float* __restrict__ det, const float* __restrict__ nsc, const float* __restrict__ esc,
    const float* __restrict__ link, const int* __restrict__ seqs, const int* __restrict__ nts, int n_nts, int max_T,
    int max_n, int cap, int gp_arg, int tab_arg, int n_scores, long long n_link, float* __restrict__ out,
    long long n_out, int* __restrict__ ids, double* __restrict__ objective, int* __restrict__ info, double* ws,
    long long ws_units) {
  constexpr int TH = 64 * NW;
  extern __shared__ __attribute__((aligned(16))) unsigned char sq_lds[];
  __shared__ double red_v[2 * NW];
  __shared__ int red_j[2 * NW];
  __shared__ int s_cnt[TH];
  __shared__ long long s_gk[GAPS ? SQ_MAXGAP : 1];  // the number of link scores of each gap
  __shared__ int s_L, s_flag;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int* sq = seqs + SQ_ROW * p;
  const int T = sq[0], so = sq[1], lo = sq[2], no = sq[3], wo = sq[5];
  const long long oo = (long long)sq[4];
  const int GP = GAPS ? gp_arg : 1;
  const int tab_lds = GAPS ? tab_arg : 1;
  const long long tab_units = GAPS ? ((long long)GP * T + 1) / 2 : 0;  // the table's room at the head of the workspace

  // ---- the launch contract: nothing of a sequence outside it is read or written but its objective and info words
  bool ok = T >= 2 && T <= SQ_MAXT && T <= max_T && GP < T && so >= 0 && lo >= 0 && no >= 0 && oo >= 0 && wo >= 0 &&
            (long long)no + T <= (long long)n_nts && (tab_lds || (long long)wo + tab_units <= ws_units);
  int bad = 0;
  if (ok) {
    for (int t = tid; t < T; t += TH) {
      const int n = nts[no + t];
      if (n < 0 || n > max_n || n > SQ_MAXN) bad = 1;
    }
  }
  if (__syncthreads_or(bad | (ok ? 0 : 1))) {
    if (tid == 0) {
      objective[p] = __builtin_nan("");
      info[4 * p] = MMMOT_SEQ_ECONTRACT;
      info[4 * p + 1] = info[4 * p + 2] = info[4 * p + 3] = 0;
    }
    return;
  }
  const int* nt = nts + no;
  int* st = (int*)sq_lds;  // frame starts [T + 1]: read at every frame step
  int* loff = tab_lds ? st + max_T + 1 : (int*)(ws + wo);  // block (g, t) of the links starts at loff[(g - 1) * T + t]
  if (tid == 0) {
    int a = 0;
    for (int t = 0; t < T; ++t) {
      st[t] = a;
      a += nt[t];
    }
    st[T] = a;
    s_L = a;
    s_flag = 0;
  }
  if (tid >= 1 && tid <= GP) {  // one thread per gap: the offsets inside the gap's run of blocks, and the run's length
    const int g = tid;
    int* row = loff + (g - 1) * T;
    long long b = 0;
    for (int t = 0; t < T; ++t) {
      row[t] = b < 0x7fffffffLL ? (int)b : 0x7fffffff;
      if (t + g < T) b += (long long)nt[t] * nt[t + g];
    }
    s_gk[g - 1] = b;
  }
  __syncthreads();
  const int L = s_L;
  long long K = 0;
  for (int g = 0; g < GP; ++g) K += s_gk[g];
  const long long state_units = ((long long)SQ_STATE_BYTES * L + 7) / 8;
  if (L < 1 || L > cap || L > SQ_MAXL || (LDS && L > SQ_LDS_CAP) || (long long)so + L > (long long)n_scores ||
      K >= 0x7fffffffLL || (long long)lo + K > n_link || oo + 3LL * L + K > n_out ||
      (!LDS && (long long)wo + tab_units + state_units > ws_units)) {
    if (tid == 0) {
      objective[p] = __builtin_nan("");
      info[4 * p] = MMMOT_SEQ_ECONTRACT;
      info[4 * p + 1] = info[4 * p + 2] = info[4 * p + 3] = 0;
    }
    return;
  }
  for (int i = T + tid; i < GP * T; i += TH) {  // the runs one after the other: K < 2^31, no sum overflows
    long long base = 0;
    const int g = i / T;
    for (int q = 0; q < g; ++q) base += s_gk[q];
    loff[i] += (int)base;
  }
  unsigned char* base;
  if constexpr (LDS) base = sq_lds + sq_frames_bytes(max_T, GP, tab_lds != 0);
  else base = (unsigned char*)(ws + wo + tab_units);
  SqState s(base, L);
  const float* lk = link + lo;
  const int SINK = 2 * L;

  for (int v = tid; v < L; v += TH) {
    s.used[v] = 0;
    s.pred[v] = -1;
    s.succ[v] = -1;
    s.inl[v] = 0.f;
    s.sdet[v] = det[so + v];
    s.snew[v] = nsc[so + v];
    s.send[v] = esc[so + v];
  }
  __syncthreads();

  int status = MMMOT_SEQ_OK, naug = 0, npass = 0, step = 0;
  const int max_pass = 2 * L + 2;
  for (int aug = 0; aug <= L; ++aug) {
    for (int v = tid; v < L; v += TH) {
      s.din[v] = INFINITY;
      s.dout[v] = INFINITY;
      s.pin[v] = -2;
      s.pout[v] = -2;
      s.pls[v] = 0.f;
    }
    __syncthreads();
    bool settled = false;
    int flo = 0, fhi = T - 1;  // the frames the next forward sweep has to visit: all of them from the empty labels
    for (int pass = 0; pass < max_pass; ++pass) {
      ++npass;
      // ---- forward sweep over the frames [flo, ..]: it ends behind fhi at the first frame that lowers nothing and
      // has no lowered frame among the GP before it
      int blo = T, bhi = -1;
      for (int t = flo; t < T; ++t) {
        const int a = st[t], n = st[t + 1] - a;
        const int t0 = max(t - GP, 0), a0 = st[t0], n0 = a - a0;  // the detections [a0, a) of the GP frames before
        int c = 0;
        if (n > 0) {
          int G = 1;  // lanes per detection k, over the detections j of the frames before
          while (G < 64 && 2 * G * n <= TH && G < n0) G <<= 1;
          const int per = TH / G, g = tid & (G - 1), slot = tid / G;
          for (int kb = 0; kb < n; kb += per) {
            const int kk = kb + slot, k = a + kk;
            const bool act = kk < n;
            double bv = INFINITY;
            int bj = 0x7fffffff;
            float bs = 0.f;
            // the hot loop, and the one place with a body per case: with GAPS bj is the global index pj; without, the
            // row j of the one block, whose 32-bit index j * n + kk keeps the next-frame kernel at its speed
            if (act) {
              if constexpr (GAPS) {
                int f = t0;
                for (int pj = a0 + g; pj < a; pj += G) {
                  for (int q = 0; q < GP && f < t - 1 && pj >= st[f + 1]; ++q) ++f;  // the frame of pj
                  const float sc = lk[(long long)loff[(t - f - 1) * T + f] + (long long)(pj - st[f]) * n + kk];
                  if (!(s.used[pj] && s.succ[pj] == k)) {
                    const double cand = s.dout[pj] + sq_cost(sc);
                    if (cand < bv) {  // pj ascending: strict < keeps the smallest index
                      bv = cand;
                      bj = pj;
                      bs = sc;
                    }
                  }
                }
              } else {
                const float* blk = lk + loff[t0];
                for (int j = g; j < n0; j += G) {
                  const int pj = a0 + j;
                  const float sc = blk[j * n + kk];  // loaded whether or not the edge is free: no wait behind the test
                  if (!(s.used[pj] && s.succ[pj] == k)) {
                    const double cand = s.dout[pj] + sq_cost(sc);
                    if (cand < bv) {  // j ascending: strict < keeps the smallest index
                      bv = cand;
                      bj = j;
                      bs = sc;
                    }
                  }
                }
              }
            }
            for (int o = G >> 1; o >= 1; o >>= 1) {
              const double ov = __shfl_xor(bv, o);
              const int oj = __shfl_xor(bj, o);
              const float os = __shfl_xor(bs, o);
              if (ov < bv || (ov == bv && oj < bj)) {
                bv = ov;
                bj = oj;
                bs = os;
              }
            }
            if (act && g == 0) {
              double best = INFINITY;
              int bp = -2;
              const double cs = sq_cost(s.snew[k]);
              if (cs < INFINITY && !(s.used[k] && s.pred[k] < 0)) {  // the source's edge, unless k starts a trajectory
                best = cs;
                bp = -1;
              }
              if (bv < best) {  // the source (node -1) wins a tie
                best = bv;
                bp = GAPS ? L + bj : L + a0 + bj;
              }
              double d = s.din[k];
              if (best < d) {
                d = best;
                s.din[k] = best;
                s.pin[k] = bp;
                s.pls[k] = bs;
                c = 1;
              }
              if (!s.used[k]) {  // in(k) -> out(k)
                const double co = d + sq_cost(s.sdet[k]);
                if (co < s.dout[k]) {
                  s.dout[k] = co;
                  s.pout[k] = k;
                  c = 1;
                }
              }
            }
          }
        }
        if (__syncthreads_or(c)) {  // dout of frame t may be lower: the frames t + 1 .. t + GP read it
          blo = min(blo, t);
          bhi = t;
          fhi = max(fhi, t + GP);
        } else if (t >= fhi) {
          break;
        }
      }
      // ---- backward sweep, the back-edges of the trajectories, over the frames [.., bhi]: it ends below blo at the
      // first frame that lowers nothing and has no lowered frame among the GP after it
      int chg = 0;
      flo = T;
      fhi = -1;
      if (naug > 0) {
        for (int t = bhi; t >= 0; --t) {
          const int a = st[t], n = st[t + 1] - a;
          int c = 0;
          for (int kk = tid; kk < n; kk += TH) {
            const int k = a + kk;
            if (s.used[k]) {
              double d = s.din[k];
              const double ci = s.dout[k] - sq_cost(s.sdet[k]);  // out(k) -> in(k): k leaves its trajectory
              if (ci < d) {
                d = ci;
                s.din[k] = ci;
                s.pin[k] = L + k;
                c = 1;
              }
              const int pk = s.pred[k];
              if (pk >= 0) {  // in(k) -> out(pred k): the link undone
                const double c2 = d - sq_cost(s.inl[k]);
                if (c2 < s.dout[pk]) {
                  s.dout[pk] = c2;
                  s.pout[pk] = k;
                  c = 1;
                }
              }
            }
          }
          if (__syncthreads_or(c)) {  // dout of the frames t - GP .. t - 1 may be lower: the frames t - GP + 1 .. t + GP - 1 read them
            fhi = max(fhi, min(T - 1, t + GP - 1));
            flo = max(0, t - GP + 1);
            blo = min(blo, t - GP);
            chg = 1;
          } else if (t <= blo) {
            break;
          }
        }
      }
      if (!chg) {
        settled = true;
        break;
      }
    }
    if (!settled) {
      status = MMMOT_SEQ_EPASS;
      break;
    }
    // ---- the sink's label: min over out(v) -> sink
    double bv = INFINITY;
    int bj = 0x7fffffff;
    for (int v = tid; v < L; v += TH) {
      if (!(s.used[v] && s.succ[v] < 0)) {
        const double c = s.dout[v] + sq_cost(s.send[v]);
        if (c < bv) {
          bv = c;
          bj = v;
        }
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const double ov = __shfl_xor(bv, o);
      const int oj = __shfl_xor(bj, o);
      if (ov < bv || (ov == bv && oj < bj)) {
        bv = ov;
        bj = oj;
      }
    }
    if (NW > 1) {
      const int par = (step & 1) * NW;  // two slot sets: the next search's writes cannot overtake this one's reads
      if (lane == 0) {
        red_v[par + wv] = bv;
        red_j[par + wv] = bj;
      }
      __syncthreads();
      bv = red_v[par];
      bj = red_j[par];
#pragma unroll
      for (int w = 1; w < NW; ++w) {
        const double ov = red_v[par + w];
        const int oj = red_j[par + w];
        if (ov < bv || (ov == bv && oj < bj)) {
          bv = ov;
          bj = oj;
        }
      }
    }
    ++step;
    if (!(bv < 0.0)) break;  // no path, or the cheapest one gains nothing: the flow is optimal
    if (aug == L) {          // more trajectories than detections: cannot be
      status = MMMOT_SEQ_EAUG;
      break;
    }
    if (tid == 0) {  // augment along the parents: every field is set by exactly one edge of the (simple) path
      int w = SINK, q = L + bj, guard = 0;
      for (; guard < max_pass; ++guard) {
        if (w != SINK) q = w < L ? s.pin[w] : s.pout[w - L];
        if (q < -1) break;  // a node without a parent: the labels were not a tree
        if (q < 0) {        // source -> in(w)
          s.pred[w] = -1;
          break;
        }
        if (w == SINK) s.succ[q - L] = -1;                 // out(v) -> sink
        else if (w >= L && q == w - L) s.used[q] = 1;      // in(v) -> out(v)
        else if (w < L && q == w + L) {                    // out(v) -> in(v): v leaves its trajectory
          s.used[w] = 0;
          s.pred[w] = -1;
          s.succ[w] = -1;
        } else if (w < L) {                                // out(a) -> in(w): a new link, of any gap
          s.pred[w] = q - L;
          s.succ[q - L] = w;
          s.inl[w] = s.pls[w];
        }                                                  // in(k) -> out(v), an undone link: both ends are set by their other edges
        w = q;
      }
      if (q != -1) s_flag = 1;
    }
    __syncthreads();
    if (s_flag) {
      status = MMMOT_SEQ_EWALK;
      break;
    }
    ++naug;
  }

  // ---- trajectory numbers: starts ranked by detection index, each trajectory walked forward by the thread of its start
  const int C = (L + TH - 1) / TH;
  const int c0 = min(L, tid * C), c1 = min(L, c0 + C);
  int* oid = ids + so;
  int cnt = 0;
  for (int v = c0; v < c1; ++v) {
    oid[v] = -1;  // every element is written, also where a walk that ended at a bound left the flow inconsistent
    cnt += s.used[v] && s.pred[v] < 0 ? 1 : 0;
  }
  s_cnt[tid] = cnt;
  __syncthreads();
  int rank = 0, total = 0;
  for (int i = 0; i < TH; ++i) {
    const int c = s_cnt[i];
    rank += i < tid ? c : 0;
    total += c;
  }
  for (int v = c0; v < c1; ++v) {
    if (s.used[v] && s.pred[v] < 0) {
      int w = v;
      for (int n = 0; n < T && w >= 0; ++n) {
        oid[w] = rank;
        w = s.succ[w];
      }
      ++rank;
    }
  }

  // ---- ortools-shaped results: [det L | new L | end L | the g = 1 blocks | .. | the g = GP blocks], every element written
  float* o = out + oo;
  for (int v = tid; v < L; v += TH) {
    const bool us = s.used[v] != 0;
    o[v] = us ? 1.f : 0.f;
    o[L + v] = us && s.pred[v] < 0 ? 1.f : 0.f;
    o[2 * L + v] = us && s.succ[v] < 0 ? 1.f : 0.f;
  }
  float* ol = o + 3LL * L;
  for (long long e = tid; e < K; e += TH) ol[e] = 0.f;
  __syncthreads();
  for (int t = tid; t < T - 1; t += TH) {
    const int a = st[t], b = st[t + 1];
    for (int v = a; v < b; ++v) {
      const int sv = s.used[v] ? s.succ[v] : -1;
      for (int g = 1; g <= GP && t + g < T; ++g) {
        const int b1 = st[t + g], n1 = st[t + g + 1] - b1;
        if (sv >= b1 && sv < b1 + n1) ol[(long long)loff[(g - 1) * T + t] + (long long)(v - a) * n1 + (sv - b1)] = 1.f;
      }
    }
  }
  // objective: wave 0 only (the same sums whatever NW), lane-strided partials then a butterfly, as the chain kernel
  if (wv == 0) {
    double acc = 0.0;
    for (int v = lane; v < L; v += 64) {
      if (s.used[v]) {
        double x = (double)s.sdet[v];
        if (s.pred[v] < 0) x += (double)s.snew[v];
        const int sv = s.succ[v];
        if (sv < 0) x += (double)s.send[v];
        else x += (double)s.inl[sv];
        acc += x;
      }
    }
#pragma unroll
    for (int o2 = 32; o2 >= 1; o2 >>= 1) acc += __shfl_xor(acc, o2);
    if (lane == 0) {
      objective[p] = status == MMMOT_SEQ_OK ? acc : __builtin_nan("");
      info[4 * p] = status;
      info[4 * p + 1] = total;
      info[4 * p + 2] = naug;
      info[4 * p + 3] = npass;
    }
  }
}

template <int NW, bool LDS, bool GAPS>
static int sq_launch(const float* det, const float* nsc, const float* esc, const float* link, const int* seqs,
                     const int* nts, int B, int n_nts, int max_T, int max_n, int max_L, int max_gap, int n_scores,
                     long long n_link, float* out, long long n_out, int* ids, double* objective, int* info, double* ws,
                     long long ws_units, hipStream_t st) {
  auto kern = associate_sequence_kernel<NW, LDS, GAPS>;
  const size_t state = LDS ? ((size_t)SQ_STATE_BYTES * max_L + 15) & ~(size_t)15 : 0;
  const bool tab_lds = sq_frames_bytes(max_T, max_gap, true) + state <= SQ_LDS_BYTES;  // always so at one gap
  const size_t lds = sq_frames_bytes(max_T, max_gap, tab_lds) + state;
  if (lds > SQ_LDS_BYTES) return MMMOT_EINVAL;
  if (lds > 64 * 1024) {  // raise this kernel's dynamic LDS limit once (160 KB per CU on gfx950)
    static const hipError_t e =
        hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SQ_LDS_BYTES);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3(B), dim3(64 * NW), lds, st, det, nsc, esc, link, seqs, nts, n_nts, max_T, max_n, max_L,
                     max_gap, tab_lds ? 1 : 0, n_scores, n_link, out, n_out, ids, objective, info, ws, ws_units);
  return mm_check(hipGetLastError());
}

// both entries: the checks, the variant (var = 0: automatic) and the launch; GAPS = false takes max_gap = 1
template <bool GAPS>
static int sq_entry(const float* det, const float* new_score, const float* end_score, const float* link, const int* seqs,
                    const int* nts, int B, int n_nts, int max_T, int max_n, int max_L, int max_gap, int n_scores,
                    long long n_link, float* out, long long n_out, int* ids, double* objective, int* info, double* ws,
                    long long ws_units, void* stream, int var) {
  if (!det || !new_score || !end_score || !link || !seqs || !nts || !out || !ids || !objective || !info || !ws)
    return MMMOT_EINVAL;
  if (B < 1 || n_nts < 2 || max_T < 2 || max_T > SQ_MAXT || max_n < 1 || max_n > SQ_MAXN || max_L < 1 || max_L > SQ_MAXL ||
      max_gap < 1 || max_gap > SQ_MAXGAP || max_gap >= max_T || n_scores < 1 || n_link < 0 || n_out < 3 || ws_units < 1 ||
      (((uintptr_t)ws) & 7u))
    return MMMOT_EINVAL;
  if (var == 0) var = (max_L <= SQ_LDS_CAP ? 3 : 1) + (max_n <= 16 ? 0 : 1);
  if (var >= 3 && max_L > SQ_LDS_CAP) return MMMOT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
#define SQ_GO(NW, LDS)                                                                                                 \
  return sq_launch<NW, LDS, GAPS>(det, new_score, end_score, link, seqs, nts, B, n_nts, max_T, max_n, max_L, max_gap,  \
                                  n_scores, n_link, out, n_out, ids, objective, info, ws, ws_units, st)
  switch (var) {
    case 1: SQ_GO(1, false);
    case 2: SQ_GO(4, false);
    case 3: SQ_GO(1, true);
    default: SQ_GO(4, true);
  }
#undef SQ_GO
}

extern "C" int mmmot_set_sequence_variant(int v) {
  if (v < 0 || v > 4) return MMMOT_EINVAL;
  g_seq_variant = v;
  return MMMOT_OK;
}

extern "C" int mmmot_set_sequence_gap_variant(int v) {
  if (v < 0 || v > 4) return MMMOT_EINVAL;
  g_seq_gap_variant = v;
  return MMMOT_OK;
}

extern "C" int mmmot_associate_sequences(const float* det, const float* new_score, const float* end_score,
                                         const float* link, const int* seqs, const int* nts, int B, int n_nts, int max_T,
                                         int max_n, int max_L, int n_scores, long long n_link, float* out, long long n_out,
                                         int* ids, double* objective, int* info, double* ws, long long ws_units,
                                         void* stream) {
  return sq_entry<false>(det, new_score, end_score, link, seqs, nts, B, n_nts, max_T, max_n, max_L, 1, n_scores, n_link,
                         out, n_out, ids, objective, info, ws, ws_units, stream, g_seq_variant);
}

extern "C" int mmmot_associate_sequences_gap(const float* det, const float* new_score, const float* end_score,
                                             const float* link, const int* seqs, const int* nts, int B, int n_nts,
                                             int max_T, int max_n, int max_L, int max_gap, int n_scores, long long n_link,
                                             float* out, long long n_out, int* ids, double* objective, int* info,
                                             double* ws, long long ws_units, void* stream) {
  return sq_entry<true>(det, new_score, end_score, link, seqs, nts, B, n_nts, max_T, max_n, max_L, max_gap, n_scores,
                        n_link, out, n_out, ids, objective, info, ws, ws_units, stream, g_seq_gap_variant);
}
