// Stand-alone host program for a sanitizer run of the argument-checking host side of mmmot_stitch_tracks
// (mmmot_amd/csrc/stitch_tracks.hip; csrc/assign.hip holds the pair solver it queues).  CPU only: every call below is
// answered before any launch, so it needs no GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined mmmot_amd/csrc/stitch_tracks.hip mmmot_amd/csrc/assign.hip \
//       tools/stitch_tracks_argcheck.cpp -fsanitize=address,undefined -o /tmp/stitch_tracks_argcheck \
//       && /tmp/stitch_tracks_argcheck
//
// Prints one line per group and returns non-zero on the first wrong answer; the sanitizers abort on their own findings.
#include <climits>
#include <cstdio>
#include <limits>
#include <vector>

#include "../include/mmmot_hip.h"

static int failures = 0;

static void expect(int got, int want, const char* what) {
  if (got != want) {
    std::printf("FAIL %s: returned %d, expected %d\n", what, got, want);
    ++failures;
  }
}

struct Sizes {
  int L, F, S, T;
  long n_link;
  int max_k, min_dt, max_dt, min_rows, mode;
  double ratio, penalty;
};

int main() {
  // real host arrays stand in for the device pointers: the checks never read through them
  const Sizes good = {2, 3, 1, 2, 4, 2, 1, 30, 3, 0, 0.0, 0.0};
  std::vector<float> det(good.L * 12, 1.f), vel(good.L * 4, 0.f), links(good.n_link);
  std::vector<int> ids = {1, 2}, fs = {0, 1, 1, 2}, no = {0, 1, 2}, ss = {0, 3}, ks = {0, 2}, pairs = {2, 2, 0, 0};
  std::vector<int> out_ids(good.L), next(good.L), info(4 * good.S);
  std::vector<double> r2(2 * (MMMOT_STITCH_MAX_DT + 1), 1.0), inv_r2(r2), objective(good.S);
  std::vector<double> xf0(good.F * MMMOT_FILL_REC, 0.0);
  std::vector<double> work8((MMMOT_STITCH_WORK(good.L, good.F, good.S, good.T, good.n_link) + 1) / 2);  // 8-byte aligned
  const int NP = 15;
  void* p[NP] = {det.data(), ids.data(), fs.data(), no.data(), ss.data(), ks.data(), pairs.data(), r2.data(),
                 inv_r2.data(), work8.data(), out_ids.data(), next.data(), links.data(), objective.data(), info.data()};
  auto call = [&](void** q, const Sizes& z, bool extras) {
    return mmmot_stitch_tracks((const float*)q[0], (const int*)q[1], (const int*)q[2], (const int*)q[3], (const int*)q[4],
                               extras ? vel.data() : nullptr, extras ? xf0.data() : nullptr, (const int*)q[5],
                               (const int*)q[6], (const double*)q[7], (const double*)q[8], z.L, z.F, z.S, z.T, z.n_link,
                               z.max_k, z.min_dt, z.max_dt, z.min_rows, z.mode, z.ratio, z.penalty, (int*)q[9],
                               (int*)q[10], (int*)q[11], (float*)q[12], (double*)q[13], (int*)q[14], nullptr);
  };

  for (int i = 0; i < NP; ++i)
    for (bool extras : {false, true}) {
      void* q[NP];
      for (int j = 0; j < NP; ++j) q[j] = j == i ? nullptr : p[j];
      expect(call(q, good, extras), MMMOT_EINVAL, "a null pointer");
    }
  std::printf("null pointers with L > 0 and F > 0: refused (vel and xf0 may be null)\n");

  {
    void* q[NP];
    for (int j = 0; j < NP; ++j) q[j] = p[j];
    q[9] = (char*)work8.data() + 4;
    expect(call(q, good, false), MMMOT_EINVAL, "work not 8-byte aligned");
  }
  Sizes z;
  for (int s : {0, -1, INT_MIN}) z = good, z.S = s, expect(call(p, z, false), MMMOT_EINVAL, "S < 1");
  for (int v : {-1, INT_MIN}) {
    z = good, z.L = v, expect(call(p, z, false), MMMOT_EINVAL, "L < 0");
    z = good, z.F = v, expect(call(p, z, false), MMMOT_EINVAL, "F < 0");
    z = good, z.T = v, expect(call(p, z, false), MMMOT_EINVAL, "n_tracks < 0");
    z = good, z.n_link = v, expect(call(p, z, false), MMMOT_EINVAL, "n_link < 0");
    z = good, z.max_k = v, expect(call(p, z, false), MMMOT_EINVAL, "max_k < 0");
  }
  z = good, z.n_link = LONG_MIN, expect(call(p, z, false), MMMOT_EINVAL, "n_link = LONG_MIN");
  z = good, z.L = INT_MAX, expect(call(p, z, false), MMMOT_EINVAL, "a scratch index past 32 bits (L)");
  z = good, z.T = INT_MAX, expect(call(p, z, false), MMMOT_EINVAL, "a scratch index past 32 bits (n_tracks)");
  z = good, z.n_link = LONG_MAX, expect(call(p, z, false), MMMOT_EINVAL, "a scratch index past 64 bits (n_link)");
  z = good, z.n_link = 0x7fffffffL, expect(call(p, z, false), MMMOT_EINVAL, "a scratch index past 32 bits (n_link)");
  std::printf("S < 1, negative sizes, sizes beyond the scratch index, a misaligned work: refused\n");

  for (int v : {0, -1, INT_MIN}) z = good, z.min_dt = v, expect(call(p, z, false), MMMOT_EINVAL, "min_dt < 1");
  z = good, z.min_dt = 31, expect(call(p, z, false), MMMOT_EINVAL, "min_dt > max_dt");
  for (int v : {MMMOT_STITCH_MAX_DT + 1, INT_MAX}) z = good, z.max_dt = v, expect(call(p, z, false), MMMOT_EINVAL, "max_dt");
  for (int v : {2, -1, INT_MAX}) z = good, z.mode = v, expect(call(p, z, false), MMMOT_EINVAL, "mode outside {0, 1}");
  for (int v : {0, -1, INT_MIN}) z = good, z.min_rows = v, expect(call(p, z, false), MMMOT_EINVAL, "min_rows < 1");
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  for (double v : {-1.0, -1e-300, nan, -inf}) {
    z = good, z.ratio = v, expect(call(p, z, true), MMMOT_EINVAL, "a negative or NaN max_size_ratio");
    z = good, z.penalty = v, expect(call(p, z, true), MMMOT_EINVAL, "a negative or NaN gap_penalty");
    z = good, z.L = 0, z.penalty = v, expect(call(p, z, true), MMMOT_EINVAL, "a bad parameter with L = 0");
  }
  std::printf("dt bounds outside 1 <= min_dt <= max_dt <= %d, a bad mode, min_rows < 1, negative or NaN parameters: "
              "refused\n", MMMOT_STITCH_MAX_DT);

  void* none[NP] = {};
  z = good, z.L = 0, expect(call(none, z, false), MMMOT_OK, "L = 0, nulls");
  z = good, z.F = 0, z.mode = 1, expect(call(none, z, false), MMMOT_OK, "F = 0, nulls");
  z = good, z.L = 0, z.F = 0, z.min_dt = z.max_dt = MMMOT_STITCH_MAX_DT, expect(call(p, z, true), MMMOT_OK, "L = F = 0");
  z = good, z.L = 0, z.S = 0, expect(call(none, z, false), MMMOT_EINVAL, "L = 0, S = 0");
  std::printf("L = 0 or F = 0: a no-op that returns 0\n");

  std::printf(failures ? "%d wrong answers\n" : "all argument checks answered as documented (%d wrong)\n", failures);
  return failures ? 1 : 0;
}
