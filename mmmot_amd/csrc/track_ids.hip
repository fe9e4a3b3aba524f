// Track IDs from the assignments of PAIRS (mmmot_track_ids) and of WINDOWS of 2 .. 8 frames (mmmot_track_chain_ids)
// (reference tracking_model.py: assign_det_id :218-292, then align_id :109-216, which are written for len(det_split)
// frames), restated by detection index: one workgroup walks the B consecutive entries of ONE sequence in order, the
// lanes take the detections of a frame, and the sequence state (last ID, the stored frame and its per-detection IDs)
// lives in LDS from the first entry of the launch to the last.  "The next free ID in detection order" is a ballot and a
// prefix count.  One kernel body serves both entry points; what differs - the table row, the stride of frame_idx and the
// trailing words - sits behind a trait (PairTab, ChainTab) that the compiler resolves.
//
// Per entry (frames f_0 .. f_{T-1}, counts n_t, block [det L | new L | end L | link_0 | .. | link_{T-2}]; a pair is
// T = 2), with `same` = the stored frame is f_0 and `first` = last_id + 1 (0 at the start of a sequence):
//   frame 0     a kept detection keeps the stored ID when `same` and that ID is >= 0 (one the previous entry rejected
//               takes a fresh one, consumed although f_0 is not emitted again), else it takes the next fresh ID
//   frame t>=1  a kept detection with new = 1 takes the next fresh ID in order of j, any other kept one the ID of the one
//               row of link_{t-1} that links to it (the IDs of frame t-1 and of frame t sit in two LDS arrays that swap)
//   the entry's LAST frame is stored when !same or frame 1 keeps a detection; otherwise nothing is stored (the
//   reference's "only support check for 2 frame case" quirk: the next entry then runs as a discontinuity).
// Behind the L IDs an entry writes frame_start (= same) and last_id; a window also `stored` (TAIL = 3).
//
// The walk is a device function (track_ids_walk).  The single entry points launch one workgroup on one state; the multi
// ones (mmmot_track_ids_multi, mmmot_track_chain_ids_multi) launch one workgroup per sequence on a table of states, each
// walking its own range of the launch's entries.
#include "common.h"

#define TK_MAXN 512
#define TK_MAX_T 8
#define TK_CHAIN_ROW (3 + TK_MAX_T)

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

// entry c of the pair table [B, 4] (N, M, ..) with frame_idx [B, 2]
struct PairTab {
  static constexpr int TAIL = 2;
  const int *row, *fi;
  __device__ PairTab(const int* table, const int* frame_idx, int c) : row(table + 4 * c), fi(frame_idx + 2 * c) {}
  __device__ int frames() const { return 2; }
  __device__ int count(int t) const { return row[t]; }
  __device__ int frame(int t) const { return fi[t]; }
};

// entry c of the chain table [B, 11] (T, .., .., n_0 .. n_7) with frame_idx [B, 8]
struct ChainTab {
  static constexpr int TAIL = 3;
  const int *row, *fi;
  __device__ ChainTab(const int* table, const int* frame_idx, int c)
      : row(table + TK_CHAIN_ROW * c), fi(frame_idx + TK_MAX_T * c) {}
  __device__ int frames() const { return row[0]; }
  __device__ int count(int t) const { return row[3 + t]; }
  __device__ int frame(int t) const { return fi[t]; }
};

// the walk of one workgroup: entries [c0, c1) of the launch on ONE state, writing ids_out from word oo on
template <int NW, class Tab>
__device__ __forceinline__ void track_ids_walk(const float* __restrict__ blocks, const int* __restrict__ table,
                                               const int* __restrict__ out_off, const int* __restrict__ frame_idx,
                                               int c0, int c1, int oo, int cap, int* __restrict__ state,
                                               int* __restrict__ ids_out) {
  constexpr int NT = 64 * NW;
  __shared__ int st[TK_MAXN], ids[2][TK_MAXN], red[8], bad;
  const int tid = threadIdx.x;
  for (int i = tid; i < TK_MAXN; i += NT) st[i] = state[MMMOT_TRACK_STATE_HEAD + i];
  if (tid == 0) bad = 0;
  // the header is uniform: every thread carries it in registers
  int last_id = state[0], stored = state[1], flag = state[2], stored_n = state[3];
  __syncthreads();

  for (int c = c0; c < c1; ++c) {  // oo: this entry's place in ids_out
    const Tab tab(table, frame_idx, c);
    const int T = tab.frames();
    bool ok = T >= 2 && T <= TK_MAX_T;
    int L = 0;
    if (ok)
      for (int t = 0; t < T; ++t) {
        const int n = tab.count(t);
        ok = ok && n >= 0 && n <= cap;
        L += n;
      }
    if (!ok) {  // outside the launch's contract (the same for every thread): stop, nothing more is written
      flag |= MMMOT_TRACK_ECONTRACT;
      break;
    }
    const int f0 = tab.frame(0), fl = tab.frame(T - 1);
    const float* blk = blocks + out_off[c];
    int* o = ids_out + oo;
    const int n0 = tab.count(0);
    const bool same = stored >= 0 && stored == f0;
    if (same && stored_n != n0) flag |= MMMOT_TRACK_ECONTRACT;  // identity is the detection index: the counts must agree
    const int first = stored < 0 ? 0 : last_id + 1;

    // frame 0 -> ids[0]
    int fresh = 0;
    for (int base = 0; base < n0; base += NT) {
      const int i = base + tid;
      const bool kept = i < n0 && blk[i] == 1.f;
      const int had = (same && i < n0) ? st[i] : -1;
      const bool q = kept && had < 0;
      int tot;
      const int r = tk_rank<NW>(q, tot, red);
      if (i < n0) {
        const int id = q ? first + fresh + r : (kept ? had : -1);
        ids[0][i] = id;
        o[i] = id;
      }
      fresh += tot;
    }
    __syncthreads();

    // frames 1 .. T-1: ids[pv] holds frame t-1, ids[pv ^ 1] takes frame t
    int pv = 0, np = n0, doff = n0, keep1 = 0;
    const float* lk = blk + 3 * L;
    for (int t = 1; t < T; ++t) {
      const int nt = tab.count(t);
      const int* prev = ids[pv];
      int* cur = ids[pv ^ 1];
      int keep = 0;
      for (int base = 0; base < nt; base += NT) {
        const int j = base + tid;
        const bool kept = j < nt && blk[doff + j] == 1.f;
        const bool q = kept && blk[L + doff + j] == 1.f;
        int tot, nk;
        const int r = tk_rank<NW>(q, tot, red);
        tk_rank<NW>(kept, nk, red);
        if (j < nt) {
          int id = -1;
          if (q) {
            id = first + fresh + r;
          } else if (kept) {  // the one row of link_{t-1} that links to column j (adjacent lanes, adjacent j)
            int n = 0, src = 0;
            for (int i = 0; i < np; ++i) {
              const bool l = lk[i * nt + j] == 1.f;
              src = l ? i : src;
              n += l ? 1 : 0;
            }
            id = n == 1 ? prev[src] : -1;
            if (id < 0) bad = 1;  // plain store, the same value from every lane that writes it
          }
          cur[j] = id;
          o[doff + j] = id;
        }
        fresh += tot;
        keep += nk;
      }
      // frame t is complete before it is read as frame t-1, and frame t-1 was read before it is overwritten as t+1
      __syncthreads();
      if (t == 1) keep1 = keep;
      lk += np * nt;
      doff += nt;
      np = nt;
      pv ^= 1;
    }
    if (bad) flag |= MMMOT_TRACK_EINFEASIBLE;

    last_id = stored < 0 ? max(last_id, fresh - 1) : last_id + fresh;
    const bool store = !same || keep1 > 0;
    if (store) {  // the entry's last frame, in ids[pv] after the last swap
      for (int j = tid; j < TK_MAXN; j += NT) st[j] = j < np ? ids[pv][j] : -1;
      stored = fl;
      stored_n = np;
    }
    if (tid == 0) {
      o[L] = same ? 1 : 0;
      o[L + 1] = last_id;
      if (Tab::TAIL == 3) o[L + 2] = store ? 1 : 0;
    }
    oo += L + Tab::TAIL;
    __syncthreads();  // st and both ID arrays are free for the next entry
  }

  for (int i = tid; i < TK_MAXN; i += NT) state[MMMOT_TRACK_STATE_HEAD + i] = st[i];
  if (tid == 0) {
    state[0] = last_id;
    state[1] = stored;
    state[2] = flag;
    state[3] = stored_n;
  }
}

template <int NW, class Tab>
__global__ __launch_bounds__(64 * NW) void track_ids_kernel(const float* __restrict__ blocks,
                                                            const int* __restrict__ table,
                                                            const int* __restrict__ out_off,
                                                            const int* __restrict__ frame_idx, int B, int cap,
                                                            int* __restrict__ state, int* __restrict__ ids_out) {
  track_ids_walk<NW, Tab>(blocks, table, out_off, frame_idx, 0, B, 0, cap, state, ids_out);
}

// S states in one launch: workgroup s walks entries [seq_start[s], seq_start[s + 1]) on row s of the state table.  Its
// place in ids_out is the sum of the entries before its range, read from the table - it does not depend on what the
// other workgroups do.  An entry outside the launch's limits in front of the range leaves that place unknown: the
// stream gets MMMOT_TRACK_ECONTRACT and is not walked.
template <int NW, class Tab>
__global__ __launch_bounds__(64 * NW) void track_ids_multi_kernel(const float* __restrict__ blocks,
                                                                  const int* __restrict__ table,
                                                                  const int* __restrict__ out_off,
                                                                  const int* __restrict__ frame_idx,
                                                                  const int* __restrict__ seq_start, int B, int cap,
                                                                  int* __restrict__ states, int* __restrict__ ids_out) {
  const int s = blockIdx.x;
  const int c0 = seq_start[s], c1 = seq_start[s + 1];
  if (c0 == c1) return;  // an empty range: the stream is neither read nor written
  int* state = states + (long)s * MMMOT_TRACK_STATE_INTS;
  if (c0 < 0 || c1 > B || c0 > c1) {  // uniform over the workgroup
    if (threadIdx.x == 0) state[2] |= MMMOT_TRACK_ECONTRACT;
    return;
  }
  // every thread sums the same words (c0 is small: the entries of the streams in front)
  int oo = 0;
  bool ok = true;
  for (int c = 0; c < c0 && ok; ++c) {
    const Tab tab(table, frame_idx, c);
    const int T = tab.frames();
    ok = T >= 2 && T <= TK_MAX_T;
    for (int t = 0; ok && t < T; ++t) {
      const int n = tab.count(t);
      ok = n >= 0 && n <= cap;
      oo += n;
    }
    oo += Tab::TAIL;
  }
  if (!ok) {  // no place in ids_out can be told: nothing of this stream is walked
    if (threadIdx.x == 0) state[2] |= MMMOT_TRACK_ECONTRACT;
    return;
  }
  track_ids_walk<NW, Tab>(blocks, table, out_off, frame_idx, c0, c1, oo, cap, state, ids_out);
}

// one wave up to 128 detections a frame, as the solve; four above (max_n picks the kernel)
template <class Tab>
int launch_track_ids(const float* blocks, const int* table, const int* out_off, const int* frame_idx, int B, int max_n,
                     int* state, int* ids_out, void* stream) {
  if (!blocks || !table || !out_off || !frame_idx || !state || !ids_out) return MMMOT_EINVAL;
  if (B < 1 || max_n < 0 || max_n > TK_MAXN) return MMMOT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (max_n <= 128)
    hipLaunchKernelGGL((track_ids_kernel<1, Tab>), dim3(1), dim3(64), 0, st, blocks, table, out_off, frame_idx, B, max_n,
                       state, ids_out);
  else
    hipLaunchKernelGGL((track_ids_kernel<4, Tab>), dim3(1), dim3(256), 0, st, blocks, table, out_off, frame_idx, B, max_n,
                       state, ids_out);
  return mm_check(hipGetLastError());
}

template <class Tab>
int launch_track_ids_multi(const float* blocks, const int* table, const int* out_off, const int* frame_idx,
                           const int* seq_start, int S, int B, int max_n, int* states, int* ids_out, void* stream) {
  if (!blocks || !table || !out_off || !frame_idx || !seq_start || !states || !ids_out) return MMMOT_EINVAL;
  if (S < 1 || B < 1 || max_n < 0 || max_n > TK_MAXN) return MMMOT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (max_n <= 128)
    hipLaunchKernelGGL((track_ids_multi_kernel<1, Tab>), dim3(S), dim3(64), 0, st, blocks, table, out_off, frame_idx,
                       seq_start, B, max_n, states, ids_out);
  else
    hipLaunchKernelGGL((track_ids_multi_kernel<4, Tab>), dim3(S), dim3(256), 0, st, blocks, table, out_off, frame_idx,
                       seq_start, B, max_n, states, ids_out);
  return mm_check(hipGetLastError());
}

}  // namespace

extern "C" int mmmot_track_ids(const float* blocks, const int* pairs, const int* out_off, const int* frame_idx, int B,
                               int max_nm, int* state, int* ids_out, void* stream) {
  return launch_track_ids<PairTab>(blocks, pairs, out_off, frame_idx, B, max_nm, state, ids_out, stream);
}

extern "C" int mmmot_track_chain_ids(const float* blocks, const int* chains, const int* out_off, const int* frame_idx,
                                     int B, int max_n, int* state, int* ids_out, void* stream) {
  return launch_track_ids<ChainTab>(blocks, chains, out_off, frame_idx, B, max_n, state, ids_out, stream);
}

extern "C" int mmmot_track_ids_multi(const float* blocks, const int* pairs, const int* out_off, const int* frame_idx,
                                     const int* seq_start, int S, int B, int max_nm, int* states, int* ids_out,
                                     void* stream) {
  return launch_track_ids_multi<PairTab>(blocks, pairs, out_off, frame_idx, seq_start, S, B, max_nm, states, ids_out,
                                         stream);
}

extern "C" int mmmot_track_chain_ids_multi(const float* blocks, const int* chains, const int* out_off,
                                           const int* frame_idx, const int* seq_start, int S, int B, int max_n,
                                           int* states, int* ids_out, void* stream) {
  return launch_track_ids_multi<ChainTab>(blocks, chains, out_off, frame_idx, seq_start, S, B, max_n, states, ids_out,
                                          stream);
}
