// Track IDs from the assignments of WINDOWS of 2 .. 8 frames (reference tracking_model.py: assign_det_id :218-292, then
// align_id :109-216, which are written for len(det_split) frames), restated by detection index like track_ids.hip: one
// workgroup walks the B consecutive windows of ONE sequence in order, the lanes take the detections of a frame, and the
// sequence state (last ID, the stored frame and its per-detection IDs) lives in LDS from the first window to the last.
//
// Per window (frames f_0 .. f_{T-1}, counts n_t, block [det L | new L | end L | link_0 | .. | link_{T-2}]), with
// `same` = the stored frame is f_0 and `first` = last_id + 1 (0 at the start of a sequence):
//   frame 0     a kept detection keeps the stored ID when `same` and that ID is >= 0, else it takes the next fresh ID
//   frame t>=1  a kept detection with new = 1 takes the next fresh ID in order of j, any other kept one the ID of the one
//               row of link_{t-1} that links to it (the IDs of frame t-1 and of frame t sit in two LDS arrays that swap)
//   the window's LAST frame is stored when !same or frame 1 keeps a detection; otherwise nothing is stored (the
//   reference's "only support check for 2 frame case" quirk: the next window then runs as a discontinuity).
// For T = 2 this is track_ids_kernel plus the third trailing word.
#include "track_rank.h"  // TK_MAXN, tk_rank

#define TK_MAX_T 8
#define TK_CHAIN_ROW (3 + TK_MAX_T)

namespace {

template <int NW>
__global__ __launch_bounds__(64 * NW) void track_chain_ids_kernel(const float* __restrict__ blocks,
                                                                  const int* __restrict__ chains,
                                                                  const int* __restrict__ out_off,
                                                                  const int* __restrict__ frame_idx, int B, int cap,
                                                                  int* __restrict__ state, int* __restrict__ ids_out) {
  constexpr int NT = 64 * NW;
  __shared__ int st[TK_MAXN], ids[2][TK_MAXN], red[8], bad;
  const int tid = threadIdx.x;
  for (int i = tid; i < TK_MAXN; i += NT) st[i] = state[MMMOT_TRACK_STATE_HEAD + i];
  if (tid == 0) bad = 0;
  // the header is uniform: every thread carries it in registers
  int last_id = state[0], stored = state[1], flag = state[2], stored_n = state[3];
  __syncthreads();

  int oo = 0;  // this window's place in ids_out
  for (int c = 0; c < B; ++c) {
    const int* row = chains + TK_CHAIN_ROW * c;
    const int T = row[0];
    bool ok = T >= 2 && T <= TK_MAX_T;
    int L = 0;
    if (ok)
      for (int t = 0; t < T; ++t) {
        const int n = row[3 + t];
        ok = ok && n >= 0 && n <= cap;
        L += n;
      }
    if (!ok) {  // outside the launch's contract (the same for every thread): stop, nothing more is written
      flag |= MMMOT_TRACK_ECONTRACT;
      break;
    }
    const int f0 = frame_idx[TK_MAX_T * c], fl = frame_idx[TK_MAX_T * c + T - 1];
    const float* blk = blocks + out_off[c];
    int* o = ids_out + oo;
    const int n0 = row[3];
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
      const int nt = row[3 + t];
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
    if (store) {  // the window's last frame, in ids[pv] after the last swap
      for (int j = tid; j < TK_MAXN; j += NT) st[j] = j < np ? ids[pv][j] : -1;
      stored = fl;
      stored_n = np;
    }
    if (tid == 0) {
      o[L] = same ? 1 : 0;
      o[L + 1] = last_id;
      o[L + 2] = store ? 1 : 0;
    }
    oo += L + 3;
    __syncthreads();  // st and both ID arrays are free for the next window
  }

  for (int i = tid; i < TK_MAXN; i += NT) state[MMMOT_TRACK_STATE_HEAD + i] = st[i];
  if (tid == 0) {
    state[0] = last_id;
    state[1] = stored;
    state[2] = flag;
    state[3] = stored_n;
  }
}

}  // namespace

extern "C" int mmmot_track_chain_ids(const float* blocks, const int* chains, const int* out_off, const int* frame_idx,
                                     int B, int max_n, int* state, int* ids_out, void* stream) {
  if (!blocks || !chains || !out_off || !frame_idx || !state || !ids_out) return MMMOT_EINVAL;
  if (B < 1 || max_n < 0 || max_n > TK_MAXN) return MMMOT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (max_n <= 128)  // one wave up to 128 detections a frame, four above, as the pair kernel (max_n picks the kernel)
    hipLaunchKernelGGL(track_chain_ids_kernel<1>, dim3(1), dim3(64), 0, st, blocks, chains, out_off, frame_idx, B, max_n,
                       state, ids_out);
  else
    hipLaunchKernelGGL(track_chain_ids_kernel<4>, dim3(1), dim3(256), 0, st, blocks, chains, out_off, frame_idx, B,
                       max_n, state, ids_out);
  return mm_check(hipGetLastError());
}
