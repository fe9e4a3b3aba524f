// Track IDs from the pair assignments (reference tracking_model.py: assign_det_id :218-292, then align_id :109-216),
// restated by detection index: one workgroup walks the B consecutive pairs of ONE sequence in order, the lanes take the
// detections of a pair, and the sequence state (last ID, the stored frame and its per-detection IDs) lives in LDS from
// the first pair of the launch to the last.  "The next free ID in detection order" is a ballot and a prefix count.
//
// Per pair (N, M detections, frame indices f0, f1), with `first` = last_id + 1 (0 at the start of a sequence):
//   case a  no frame stored yet            frame-0 kept detections take first + 0, 1, ..; both frames are emitted
//   case b  the stored frame is not f0     the same with first = last_id + 1
//   case c  the stored frame is f0         a kept frame-0 detection keeps the stored ID; one the previous pair rejected
//                                          takes a fresh one in order of i (consumed although f0 is not emitted again)
//   then a kept frame-1 detection with new = 1 takes the next fresh ID in order of j, any other kept one the ID of the
//   one kept row that links to it.  Case c stores frame 1 only when it keeps a detection (the reference's quirk: the
//   next pair then runs as case b); a and b always store it.
#include "track_rank.h"  // TK_MAXN, tk_rank

namespace {

template <int NW>
__global__ __launch_bounds__(64 * NW) void track_ids_kernel(const float* __restrict__ blocks,
                                                            const int* __restrict__ pairs,
                                                            const int* __restrict__ out_off,
                                                            const int* __restrict__ frame_idx, int B, int cap,
                                                            int* __restrict__ state, int* __restrict__ ids_out) {
  constexpr int T = 64 * NW;
  __shared__ int st[TK_MAXN], id0[TK_MAXN], id1[TK_MAXN], red[8], bad;
  const int tid = threadIdx.x;
  for (int i = tid; i < TK_MAXN; i += T) st[i] = state[MMMOT_TRACK_STATE_HEAD + i];
  if (tid == 0) bad = 0;
  // the header is uniform: every thread carries it in registers
  int last_id = state[0], stored = state[1], flag = state[2], stored_n = state[3];
  __syncthreads();

  int oo = 0;  // this pair's place in ids_out
  for (int p = 0; p < B; ++p) {
    const int N = pairs[4 * p], M = pairs[4 * p + 1];
    if (N < 0 || M < 0 || N > cap || M > cap) {  // outside the launch's contract: stop, nothing more is written
      flag |= MMMOT_TRACK_ECONTRACT;
      break;
    }
    const int L = N + M, f0 = frame_idx[2 * p], f1 = frame_idx[2 * p + 1];
    const float* blk = blocks + out_off[p];
    const float* lk = blk + 3 * L;
    int* o = ids_out + oo;
    const bool same = stored >= 0 && stored == f0;  // case c
    if (same && stored_n != N) flag |= MMMOT_TRACK_ECONTRACT;  // identity is the detection index: the counts must agree
    const int first = stored < 0 ? 0 : last_id + 1;

    // frame 0
    int fresh = 0;
    for (int base = 0; base < N; base += T) {
      const int i = base + tid;
      const bool kept = i < N && blk[i] == 1.f;
      const int had = (same && i < N) ? st[i] : -1;
      const bool q = kept && had < 0;
      int tot;
      const int r = tk_rank<NW>(q, tot, red);
      if (i < N) {
        const int id = q ? first + fresh + r : (kept ? had : -1);
        id0[i] = id;
        o[i] = id;
      }
      fresh += tot;
    }
    __syncthreads();

    // frame 1
    int keep1 = 0;
    for (int base = 0; base < M; base += T) {
      const int j = base + tid;
      const bool kept = j < M && blk[N + j] == 1.f;
      const bool q = kept && blk[L + N + j] == 1.f;
      int tot, nk;
      const int r = tk_rank<NW>(q, tot, red);
      tk_rank<NW>(kept, nk, red);
      if (j < M) {
        int id = -1;
        if (q) {
          id = first + fresh + r;
        } else if (kept) {  // the one kept row that links to column j
          int n = 0, row = 0;
          for (int i = 0; i < N; ++i) {
            const bool l = lk[i * M + j] == 1.f;
            row = l ? i : row;
            n += l ? 1 : 0;
          }
          id = n == 1 ? id0[row] : -1;
          if (id < 0) bad = 1;  // plain store, the same value from every lane that writes it
        }
        id1[j] = id;
        o[N + j] = id;
      }
      fresh += tot;
      keep1 += nk;
    }
    __syncthreads();
    if (bad) flag |= MMMOT_TRACK_EINFEASIBLE;

    last_id = stored < 0 ? max(last_id, fresh - 1) : last_id + fresh;
    if (!same || keep1 > 0) {  // store frame 1 (case c with nothing kept stores nothing: the reference's quirk)
      for (int j = tid; j < TK_MAXN; j += T) st[j] = j < M ? id1[j] : -1;
      stored = f1;
      stored_n = M;
    }
    if (tid == 0) {
      o[L] = same ? 1 : 0;
      o[L + 1] = last_id;
    }
    oo += L + 2;
    __syncthreads();
  }

  for (int i = tid; i < TK_MAXN; i += T) state[MMMOT_TRACK_STATE_HEAD + i] = st[i];
  if (tid == 0) {
    state[0] = last_id;
    state[1] = stored;
    state[2] = flag;
    state[3] = stored_n;
  }
}

}  // namespace

extern "C" int mmmot_track_ids(const float* blocks, const int* pairs, const int* out_off, const int* frame_idx, int B,
                               int max_nm, int* state, int* ids_out, void* stream) {
  if (!blocks || !pairs || !out_off || !frame_idx || !state || !ids_out) return MMMOT_EINVAL;
  if (B < 1 || max_nm < 0 || max_nm > TK_MAXN) return MMMOT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (max_nm <= 128)  // one wave up to 128 detections a frame, as the solve; four above (max_nm picks the kernel)
    hipLaunchKernelGGL(track_ids_kernel<1>, dim3(1), dim3(64), 0, st, blocks, pairs, out_off, frame_idx, B, max_nm,
                       state, ids_out);
  else
    hipLaunchKernelGGL(track_ids_kernel<4>, dim3(1), dim3(256), 0, st, blocks, pairs, out_off, frame_idx, B, max_nm,
                       state, ids_out);
  return mm_check(hipGetLastError());
}
