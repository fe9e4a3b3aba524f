// Tracklet stitching: every track of a sequence is one node, a tail is joined to the head of a later track when the
// constant-velocity prediction of one reaches the other, one to one (see include/mmmot_hip.h: mmmot_stitch_tracks;
// DESIGN section 12c, whose operation order this file follows).
//
// Seven launches of this file and the pair solver's one, whatever the number of rows, frames, sequences or tracks:
//   sk_check   one thread per table entry: ft_check_entry of track_links.h, and the shape of k_start / pairs
//   sk_link    one thread per detection: its frame, duplicates, its successor; the predecessor is the successor
//              scattered back
//   sk_heads   one thread per detection: a row with an ID and no predecessor heads a track; heads are counted per listed
//              frame and per sequence by integer atomics (counts, so no word depends on their order)
//   sk_tracks  one thread per detection: a head finds its rank (the heads of the frames before it, the heads of its own
//              frame in front of it), walks to its tail and stores the track's rows, head and tail records; one thread
//              per sequence settles the status and the solver's pair row
//   sk_cost    SK_PARTS workgroups per sequence: the head records of a tile of SK_TILE tracks are staged in LDS once,
//              the threads stride over (tail, head) with consecutive lanes on consecutive heads
//   (solver)   mmmot_associate_pairs over the link blocks with all-zero det / new / end scores
//   sk_match   one thread per track: the head its tail was matched to, scattered back as the predecessor track
//   sk_merge   one thread per detection: the root of its track's chain, out_ids, next, the counters
// Integer atomics only; every output word has one writer, so two calls give the same bits.  fp64 with every product and
// sum rounded on its own (`#pragma clang fp contract(off)`), one rounding to fp32 at the store.
#include "common.h"
#include "track_links.h"

#define SK_THREADS 256
#define SK_TILE 256   // head records per LDS tile
#define SK_PARTS 8    // workgroups per sequence in sk_cost: the tails are split among them
#define SK_REC 12     // doubles per track: head P, head V, tail P, tail V
#define SK_BAD_FRAMES 1
#define SK_BAD_TRACKS 2

// the tables behind the SK_REC T doubles of the scratch (MMMOT_STITCH_WORK counts the same words)
struct sk_work {
  double* rec;
  int *flag, *frame_heads, *zeros;          // set to 0 by one memset: flag (2 words), [F], [2 T] (the solver's scores)
  int *pred, *prev_t, *next_t;              // set to -1 by one memset: [L], [T], [T]
  int *frame, *succ, *track_of;             // [L] each
  int *t_head, *t_tail, *t_rows, *t_hno, *t_tno;  // [T] each
  int *wpairs, *out_off;                    // [4 S], [S]
  float* sol;                               // [6 T + n_link]: what the solver writes
};

__host__ __device__ __forceinline__ sk_work sk_split(int* work, long L, long F, long S, long T) {
  sk_work w;
  w.rec = (double*)work;
  int* t = work + 2 * SK_REC * T;
  w.flag = t, w.frame_heads = t + 2, w.zeros = w.frame_heads + F;
  w.pred = w.zeros + 2 * T, w.prev_t = w.pred + L, w.next_t = w.prev_t + T;
  w.frame = w.next_t + T, w.succ = w.frame + L, w.track_of = w.succ + L;
  w.t_head = w.track_of + L, w.t_tail = w.t_head + T, w.t_rows = w.t_tail + T, w.t_hno = w.t_rows + T;
  w.t_tno = w.t_hno + T;
  w.wpairs = w.t_tno + T, w.out_off = w.wpairs + 4 * S;
  w.sol = (float*)(w.out_off + S);
  return w;
}

struct sk_dims {
  int L, F, S, T;
  int cap;  // the solver's launch serves K <= cap = min(max_k, MMMOT_STITCH_MAXK)
  long n_link;
};

// the status a sequence gets from its head count kd, against the host's count K and the limits
__device__ __forceinline__ int sk_count_status(int kd, int K, int cap) {
  return (kd != K || (kd > cap && kd <= MMMOT_STITCH_MAXK) ? MMMOT_FILL_ECONTRACT : 0) |
         (kd > MMMOT_STITCH_MAXK ? MMMOT_STITCH_ETOOMANY : 0);
}

__global__ __launch_bounds__(SK_THREADS) void sk_check_kernel(const int* __restrict__ frame_start,
                                                              const int* __restrict__ frame_no,
                                                              const int* __restrict__ seq_start,
                                                              const int* __restrict__ k_start,
                                                              const int* __restrict__ pairs, sk_dims n,
                                                              int* __restrict__ work, int* __restrict__ info) {
  const int i = blockIdx.x * SK_THREADS + threadIdx.x;
  const sk_work w = sk_split(work, n.L, n.F, n.S, n.T);
  ft_check_entry(i, frame_start, frame_no, seq_start, n.L, n.F, n.S, w.flag, info);
  if (i < n.S) {
    // k_start is a prefix table that ends at T; pair row i is (K, K, 2 k_start[i], sum of the K^2 before it)
    const int a = k_start[i], b = k_start[i + 1];
    bool bad = a < 0 || a > b || b > n.T || (i == 0 && a != 0) || (i == n.S - 1 && b != n.T);
    if (!bad) {
      const long K = (long)b - a, lo = pairs[4 * (long)i + 3];
      bad = pairs[4 * (long)i] != K || pairs[4 * (long)i + 1] != K || pairs[4 * (long)i + 2] != 2 * (long)a || lo < 0 ||
            (i == 0 && lo != 0);
      const long end = lo + K * K;
      bad = bad || (i == n.S - 1 ? end != n.n_link : end != (long)pairs[4 * (long)i + 7]);
    }
    if (bad) atomicOr(w.flag, SK_BAD_TRACKS);
  }
}

__global__ __launch_bounds__(SK_THREADS) void sk_link_kernel(const int* __restrict__ ids,
                                                             const int* __restrict__ frame_start,
                                                             const int* __restrict__ seq_start, sk_dims n,
                                                             int* __restrict__ work, int* __restrict__ info) {
  const int i = blockIdx.x * SK_THREADS + threadIdx.x;
  const sk_work w = sk_split(work, n.L, n.F, n.S, n.T);
  if (i >= n.L || *w.flag) return;
  const int pa = ft_last_le(frame_start, n.F, i);
  const int s = ft_last_le(seq_start, n.S, pa);
  const int id = ids[i];
  int sj = -1;
  if (id >= 0) {
    if (ft_dup_in_frame(ids, frame_start, pa, i, id)) atomicOr(&info[4 * s], MMMOT_FILL_EDUP);
    int pb;
    sj = ft_successor(ids, frame_start, pa, seq_start[s + 1], id, pb);
    if (sj >= 0) w.pred[sj] = i;  // sj in (i, L): found through a checked frame_start
  }
  w.frame[i] = pa;
  w.succ[i] = sj;
}

__global__ __launch_bounds__(SK_THREADS) void sk_heads_kernel(const int* __restrict__ ids,
                                                              const int* __restrict__ seq_start, sk_dims n,
                                                              int* __restrict__ work, int* __restrict__ info) {
  const int i = blockIdx.x * SK_THREADS + threadIdx.x;
  const sk_work w = sk_split(work, n.L, n.F, n.S, n.T);
  if (i >= n.L || *w.flag) return;
  if (ids[i] < 0 || w.pred[i] >= 0) return;
  const int pa = w.frame[i];
  atomicAdd(&w.frame_heads[pa], 1);
  atomicAdd(&info[4 * ft_last_le(seq_start, n.S, pa) + 1], 1);
}

// (x, y, z[, 1]) M, columns 0..2, M the row-vector 4x4 of a record: ((x M0j + y M1j) + z M2j) [+ M3j]
__device__ __forceinline__ void sk_affine(const double* __restrict__ M, double x, double y, double z, bool point,
                                          double* __restrict__ o) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    double s = x * M[0 + j] + y * M[4 + j];
    s = s + z * M[8 + j];
    o[j] = point ? s + M[12 + j] : s;
  }
}

// P and V of one row into o[0..5]
__device__ __forceinline__ void sk_record(const float* __restrict__ det, const float* __restrict__ vel,
                                          const double* __restrict__ xf0, int row, int fr, double* __restrict__ o) {
  const float* __restrict__ a = det + (long)row * 12;
  const double x = (double)a[7], y = (double)a[8], z = (double)a[9];
  double vx = 0.0, vy = 0.0, vz = 0.0;
  if (vel) vx = (double)vel[(long)row * 4], vy = (double)vel[(long)row * 4 + 1], vz = (double)vel[(long)row * 4 + 2];
  if (xf0) {
    const double* __restrict__ M = xf0 + (long)fr * MMMOT_FILL_REC;
    sk_affine(M, x, y, z, true, o);
    sk_affine(M, vx, vy, vz, false, o + 3);
  } else {
    o[0] = x, o[1] = y, o[2] = z, o[3] = vx, o[4] = vy, o[5] = vz;
  }
}

__global__ __launch_bounds__(SK_THREADS) void sk_tracks_kernel(const float* __restrict__ det,
                                                               const int* __restrict__ ids,
                                                               const int* __restrict__ frame_start,
                                                               const int* __restrict__ frame_no,
                                                               const int* __restrict__ seq_start,
                                                               const float* __restrict__ vel,
                                                               const double* __restrict__ xf0,
                                                               const int* __restrict__ k_start,
                                                               const int* __restrict__ pairs, sk_dims n,
                                                               int* __restrict__ work, int* __restrict__ info) {
  const int i = blockIdx.x * SK_THREADS + threadIdx.x;
  const sk_work w = sk_split(work, n.L, n.F, n.S, n.T);
  const int flag = *w.flag;
  if (i < n.S) {
    // the sequence's status is settled here: the bits of the launches before or, without any, the head count against
    // k_start and the limits.  The threads of its heads below decide by the same values, whether they read info[4 i]
    // before or after this store
    int st = MMMOT_FILL_ECONTRACT, lo = 0, K = 0, so = 0;
    if (!flag) {
      const int kd = info[4 * i + 1];
      K = k_start[i + 1] - k_start[i];
      so = 2 * k_start[i], lo = pairs[4 * i + 3];
      st = info[4 * i];  // the earlier bits: final since the launch before; with one of them the heads are not counted on
      if (!st && (st = sk_count_status(kd, K, n.cap)) != 0) info[4 * i] = st;
    }
    const bool run = st == 0;
    w.wpairs[4 * i] = run ? K : 0, w.wpairs[4 * i + 1] = run ? K : 0;
    w.wpairs[4 * i + 2] = run ? so : 0, w.wpairs[4 * i + 3] = run ? lo : 0;
    w.out_off[i] = run ? 3 * so + lo : 0;  // behind the 6 K' words of the sequences before and their link blocks
  }
  if (i >= n.L || flag) return;
  if (ids[i] < 0 || w.pred[i] >= 0) return;
  const int pa = w.frame[i];
  const int s = ft_last_le(seq_start, n.S, pa);
  const int kd = info[4 * s + 1], k0 = k_start[s];
  if (info[4 * s] != 0 || sk_count_status(kd, k_start[s + 1] - k0, n.cap) != 0) return;
  int rank = 0;
  for (int q = seq_start[s]; q < pa; ++q) rank += w.frame_heads[q];
  for (int c = frame_start[pa]; c < i; ++c) rank += ids[c] >= 0 && w.pred[c] < 0;
  const int k = k0 + rank;  // < k_start[s + 1]: the sequence has kd heads
  int tail = i, rows = 0;
  for (int c = i; c >= 0; c = w.succ[c]) {  // succ strictly increases: the walk ends
    w.track_of[c] = k;
    tail = c, ++rows;
  }
  const int ft = w.frame[tail];
  w.t_head[k] = i, w.t_tail[k] = tail, w.t_rows[k] = rows;
  w.t_hno[k] = frame_no[pa], w.t_tno[k] = frame_no[ft];
  double* __restrict__ rec = w.rec + (long)k * SK_REC;
  sk_record(det, vel, xf0, i, pa, rec);
  sk_record(det, vel, xf0, tail, ft, rec + 6);
}

// max(a, b) <= ratio * min(a, b), written so that a NaN on either side fails (gl_size_ok of gate_links.hip)
__device__ __forceinline__ bool sk_size_ok(float a, float b, double ratio) {
#pragma clang fp contract(off)
  const bool gt = a > b;
  const double hi = (double)(gt ? a : b), lo = (double)(gt ? b : a);
  const double lim = ratio * lo;
  return hi <= lim;
}

// e0 e0 + e2 e2 (+ e1 e1 last in mode 1)
__device__ __forceinline__ double sk_norm(double e0, double e1, double e2, int mode) {
#pragma clang fp contract(off)
  const double xx = e0 * e0, zz = e2 * e2;
  double d2 = xx + zz;
  if (mode == 1) {
    const double yy = e1 * e1;
    d2 = d2 + yy;
  }
  return d2;
}

struct sk_gate {
  int min_dt, max_dt, min_rows, mode;
  double max_size_ratio, gap_penalty;
};

__global__ __launch_bounds__(SK_THREADS) void sk_cost_kernel(const float* __restrict__ det,
                                                             const int* __restrict__ pairs,
                                                             const double* __restrict__ r2tab,
                                                             const double* __restrict__ inv_r2tab, int has_vel,
                                                             sk_dims n, sk_gate g, int* __restrict__ work,
                                                             const int* __restrict__ info, float* __restrict__ links) {
#pragma clang fp contract(off)
  __shared__ double hp[3][SK_TILE], hv[3][SK_TILE];
  __shared__ float hd[3][SK_TILE];
  __shared__ int hno[SK_TILE], hvel[SK_TILE];
  const sk_work w = sk_split(work, n.L, n.F, n.S, n.T);
  const int s = blockIdx.x, part = blockIdx.y, tid = threadIdx.x;
  const int flag = *w.flag;
  const float qnan = __builtin_nanf("");
  if (flag & SK_BAD_TRACKS) {  // no block can be told from the next: the whole of links is absent
    const long step = (long)gridDim.x * SK_PARTS * SK_THREADS;
    for (long e = ((long)s * SK_PARTS + part) * SK_THREADS + tid; e < n.n_link; e += step) links[e] = qnan;
    return;
  }
  // checked by sk_check: K >= 0 and [off, off + K K) inside links
  const int K = pairs[4 * s];
  const long off = pairs[4 * s + 3];
  const int per = (K + SK_PARTS - 1) / SK_PARTS;
  const int i0 = min(K, part * per), i1 = min(K, i0 + per);
  if (flag || info[4 * s] != 0) {
    const long a = off + (long)i0 * K, b = off + (long)i1 * K;
    for (long e = a + tid; e < b; e += SK_THREADS) links[e] = qnan;
    return;
  }
  const int k0 = w.wpairs[4 * s + 2] >> 1;  // k_start[s]
  for (int c0 = 0; c0 < K; c0 += SK_TILE) {
    const int cw = min(SK_TILE, K - c0);
    __syncthreads();  // the tile's readers of the round before
    for (int k = tid; k < cw; k += SK_THREADS) {
      const int t = k0 + c0 + k;
      const double* __restrict__ rec = w.rec + (long)t * SK_REC;
      const float* __restrict__ d = det + (long)w.t_head[t] * 12;
#pragma unroll
      for (int j = 0; j < 3; ++j) hp[j][k] = rec[j], hv[j][k] = rec[3 + j], hd[j][k] = d[4 + j];
      hno[k] = w.t_hno[t];
      hvel[k] = has_vel && w.t_rows[t] >= g.min_rows;
    }
    __syncthreads();
    const long n_ent = (long)(i1 - i0) * cw;
    for (long e = tid; e < n_ent; e += SK_THREADS) {
      const int i = i0 + (int)(e / cw), k = (int)(e - (long)(i - i0) * cw);
      const int t = k0 + i;
      const long long dt = (long long)hno[k] - (long long)w.t_tno[t];
      float sc = qnan;
      if (dt >= g.min_dt && dt <= g.max_dt) {
        const double* __restrict__ rec = w.rec + (long)t * SK_REC + 6;
        const bool tv = has_vel && w.t_rows[t] >= g.min_rows, hv_ok = hvel[k] != 0;
        const double d = (double)dt;
        const int m = tv || hv_ok ? 0 : 1;
        const double r2 = r2tab[(long)m * (g.max_dt + 1) + dt], inv_r2 = inv_r2tab[(long)m * (g.max_dt + 1) + dt];
        double ef = 0.0, eb = 0.0, d2;
        if (tv) {
          double e3[3];
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const double step = d * rec[3 + j];
            const double at = rec[j] + step;
            e3[j] = hp[j][k] - at;
          }
          ef = sk_norm(e3[0], e3[1], e3[2], g.mode);
        }
        if (hv_ok) {
          double e3[3];
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const double step = d * hv[j][k];
            const double at = hp[j][k] - step;
            e3[j] = rec[j] - at;
          }
          eb = sk_norm(e3[0], e3[1], e3[2], g.mode);
        }
        bool pass;
        if (tv && hv_ok) {
          pass = ef <= r2 && eb <= r2;  // false for a NaN on either side
          d2 = eb > ef ? eb : ef;
        } else {
          if (tv) d2 = ef;
          else if (hv_ok) d2 = eb;
          else d2 = sk_norm(hp[0][k] - rec[0], hp[1][k] - rec[1], hp[2][k] - rec[2], g.mode);
          pass = d2 <= r2;
        }
        if (g.max_size_ratio > 0.0) {
          const float* __restrict__ a = det + (long)w.t_tail[t] * 12;
          pass = pass && sk_size_ok(a[4], hd[0][k], g.max_size_ratio) && sk_size_ok(a[5], hd[1][k], g.max_size_ratio) &&
                 sk_size_ok(a[6], hd[2][k], g.max_size_ratio);
        }
        if (pass) {
          const double u = d2 * inv_r2;
          const double near = 1.0 - u;
          const double gap = d - 1.0;
          const double pen = g.gap_penalty * gap;
          sc = (float)(near - pen);
        }
      }
      links[off + (long)i * K + c0 + k] = sc;
    }
  }
}

__global__ __launch_bounds__(SK_THREADS) void sk_match_kernel(const int* __restrict__ k_start, sk_dims n,
                                                              int* __restrict__ work, int* __restrict__ info) {
  const int t = blockIdx.x * SK_THREADS + threadIdx.x;
  const sk_work w = sk_split(work, n.L, n.F, n.S, n.T);
  if (t >= n.T || *w.flag) return;
  const int s = ft_last_le(k_start, n.S, t);  // checked by sk_check; sequences without tracks are skipped
  const int K = w.wpairs[4 * s];              // 0: the sequence has a status, the solver wrote nothing
  const int k0 = k_start[s], i = t - k0;
  if (i >= K) return;
  // the solver's link section [K][K] behind det | new | end of 2 K words each: a 1 marks the matched head
  const float* __restrict__ row = w.sol + w.out_off[s] + 6 * (long)K + (long)i * K;
  int j = 0;
  while (j < K && row[j] != 1.f) ++j;
  if (j == K) return;
  w.next_t[t] = k0 + j;
  w.prev_t[k0 + j] = t;  // one to one: a single writer
  atomicAdd(&info[4 * s + 2], 1);
}

__global__ __launch_bounds__(SK_THREADS) void sk_merge_kernel(const int* __restrict__ ids,
                                                              const int* __restrict__ seq_start, sk_dims n,
                                                              int* __restrict__ work, int* __restrict__ out_ids,
                                                              int* __restrict__ next, int* __restrict__ info) {
  const int i = blockIdx.x * SK_THREADS + threadIdx.x;
  const sk_work w = sk_split(work, n.L, n.F, n.S, n.T);
  const bool bad = *w.flag != 0;
  if (i < n.S) {  // no row thread reads or adds to the counters of a sequence with a status
    if (bad) info[4 * i] = MMMOT_FILL_ECONTRACT;
    if (bad || info[4 * i] != 0) info[4 * i + 1] = info[4 * i + 2] = info[4 * i + 3] = 0;
  }
  if (i >= n.L) return;
  const int id = ids[i];
  int oid = id, nx = -1;
  if (!bad && id >= 0) {
    const int s = ft_last_le(seq_start, n.S, w.frame[i]);
    if (info[4 * s] == 0) {  // final since sk_tracks
      const int t = w.track_of[i];
      int r = t;
      // head frame numbers strictly decrease towards the root, so the walk ends; the bound only guards the scratch
      for (int c = 0; c < MMMOT_STITCH_MAXK && w.prev_t[r] >= 0; ++c) r = w.prev_t[r];
      oid = ids[w.t_head[r]];
      if (oid != id) atomicAdd(&info[4 * s + 3], 1);
      if (i == w.t_tail[t] && w.next_t[t] >= 0) nx = w.t_head[w.next_t[t]];
    }
  }
  out_ids[i] = oid;
  next[i] = nx;
}

extern "C" int mmmot_stitch_tracks(const float* det, const int* ids, const int* frame_start, const int* frame_no,
                                   const int* seq_start, const float* vel, const double* xf0, const int* k_start,
                                   const int* pairs, const double* r2, const double* inv_r2, int L, int F, int S,
                                   int n_tracks, long n_link, int max_k, int min_dt, int max_dt, int min_rows, int mode,
                                   double max_size_ratio, double gap_penalty, int* work, int* out_ids, int* next,
                                   float* links, double* objective, int* info, void* hip_stream) {
  if (S < 1 || L < 0 || F < 0 || n_tracks < 0 || n_link < 0 || max_k < 0) return MMMOT_EINVAL;
  if (min_dt < 1 || max_dt < min_dt || max_dt > MMMOT_STITCH_MAX_DT || (mode != 0 && mode != 1) || min_rows < 1)
    return MMMOT_EINVAL;
  if (!(max_size_ratio >= 0.0) || !(gap_penalty >= 0.0)) return MMMOT_EINVAL;  // NaN included
  if (L == 0 || F == 0) return MMMOT_OK;
  if (!det || !ids || !frame_start || !frame_no || !seq_start || !k_start || !pairs || !r2 || !inv_r2 || !work ||
      !out_ids || !next || !links || !objective || !info)
    return MMMOT_EINVAL;
  // n_link first: the sum below must not overflow
  if (((size_t)work & 7) != 0 || n_link > 0x7fffffffL || MMMOT_STITCH_WORK(L, F, S, n_tracks, n_link) > 0x7fffffffL)
    return MMMOT_EINVAL;
  hipStream_t st = (hipStream_t)hip_stream;
  const sk_work w = sk_split(work, L, F, S, n_tracks);
  sk_dims n;
  n.L = L, n.F = F, n.S = S, n.T = n_tracks, n.n_link = n_link;
  n.cap = max_k < 1 ? 1 : (max_k > MMMOT_STITCH_MAXK ? MMMOT_STITCH_MAXK : max_k);
  sk_gate g;
  g.min_dt = min_dt, g.max_dt = max_dt, g.min_rows = min_rows, g.mode = mode;
  g.max_size_ratio = max_size_ratio, g.gap_penalty = gap_penalty;
  int rc = mm_check(hipMemsetAsync(w.flag, 0, sizeof(int) * (size_t)(w.pred - w.flag), st));
  if (rc != MMMOT_OK) return rc;
  rc = mm_check(hipMemsetAsync(w.pred, 0xff, sizeof(int) * (size_t)(w.frame - w.pred), st));
  if (rc != MMMOT_OK) return rc;
  rc = mm_check(hipMemsetAsync(info, 0, sizeof(int) * 4 * (size_t)S, st));
  if (rc != MMMOT_OK) return rc;
  const int n_tab = F > S ? F : S, n_row = L > S ? L : S;
  const auto blocks = [](long m) { return dim3((unsigned)(m > SK_THREADS ? (m + SK_THREADS - 1) / SK_THREADS : 1)); };
  hipLaunchKernelGGL(sk_check_kernel, blocks(n_tab), dim3(SK_THREADS), 0, st, frame_start, frame_no, seq_start, k_start,
                     pairs, n, work, info);
  hipLaunchKernelGGL(sk_link_kernel, blocks(L), dim3(SK_THREADS), 0, st, ids, frame_start, seq_start, n, work, info);
  hipLaunchKernelGGL(sk_heads_kernel, blocks(L), dim3(SK_THREADS), 0, st, ids, seq_start, n, work, info);
  hipLaunchKernelGGL(sk_tracks_kernel, blocks(n_row), dim3(SK_THREADS), 0, st, det, ids, frame_start, frame_no,
                     seq_start, vel, xf0, k_start, pairs, n, work, info);
  hipLaunchKernelGGL(sk_cost_kernel, dim3((unsigned)S, SK_PARTS), dim3(SK_THREADS), 0, st, det, pairs, r2, inv_r2,
                     (int)(vel != nullptr), n, g, work, info, links);
  rc = mm_check(hipGetLastError());
  if (rc != MMMOT_OK) return rc;
  // the pair solver over the sequences' blocks: g_ij = link_ij with det, new and end all zero (one zeroed table serves
  // the three); a sequence with a status has the pair row (0, 0, 0, 0) and gets a NaN objective, nothing else
  const float* zeros = (const float*)w.zeros;
  rc = mmmot_associate_pairs(zeros, zeros, zeros, links, w.wpairs, S, n.cap, w.sol, w.out_off, objective, hip_stream);
  if (rc != MMMOT_OK) return rc;
  hipLaunchKernelGGL(sk_match_kernel, blocks(n_tracks), dim3(SK_THREADS), 0, st, k_start, n, work, info);
  hipLaunchKernelGGL(sk_merge_kernel, blocks(n_row), dim3(SK_THREADS), 0, st, ids, seq_start, n, work, out_ids, next,
                     info);
  return mm_check(hipGetLastError());
}

