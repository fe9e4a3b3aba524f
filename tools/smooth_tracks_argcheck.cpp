// Stand-alone host program for a sanitizer run of the argument-checking host side of mmmot_smooth_tracks
// (mmmot_amd/csrc/smooth_tracks.hip).  CPU only: every call below is answered before any launch, so it needs no GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined mmmot_amd/csrc/smooth_tracks.hip tools/smooth_tracks_argcheck.cpp \
//       -fsanitize=address,undefined -o /tmp/smooth_tracks_argcheck && /tmp/smooth_tracks_argcheck
//
// Prints one line per group and returns non-zero on the first wrong answer; the sanitizers abort on their own findings.
#include <climits>
#include <cmath>
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

int main() {
  // real host arrays stand in for the device pointers: the checks never read through them
  const int L = 2, F = 3, S = 1;
  std::vector<float> det(L * 12, 1.f), out(L * 12, 0.f), vel(L * 4, 0.f);
  std::vector<int> ids = {1, 1}, fs = {0, 1, 1, 2}, no = {0, 1, 2}, ss = {0, 3}, obs = {1, 1}, info(4 * S);
  std::vector<double> work8((MMMOT_SMOOTH_WORK(L) + 1) / 2), xf0(F * MMMOT_FILL_REC, 0.0);  // doubles: 8-byte aligned
  void* p[8] = {det.data(), ids.data(), fs.data(), no.data(), ss.data(), work8.data(), out.data(), info.data()};
  const double good[8] = {0.01, 0.04, 1.0, 0.001, 0.01, 0.04, 0.0, 0.01};
  auto call = [&](void** q, int l, int f, int s, const double* prm, int flip, bool extras) {
    return mmmot_smooth_tracks((const float*)q[0], (const int*)q[1], (const int*)q[2], (const int*)q[3], (const int*)q[4],
                               extras ? obs.data() : nullptr, extras ? xf0.data() : nullptr, l, f, s, prm[0], prm[1],
                               prm[2], prm[3], prm[4], prm[5], prm[6], prm[7], flip, (int*)q[5], (float*)q[6],
                               extras ? vel.data() : nullptr, (int*)q[7], nullptr);
  };

  for (int i = 0; i < 8; ++i)
    for (bool extras : {false, true}) {
      void* q[8];
      for (int j = 0; j < 8; ++j) q[j] = j == i ? nullptr : p[j];
      expect(call(q, L, F, S, good, 0, extras), MMMOT_EINVAL, "a null pointer");
    }
  std::printf("null pointers with L > 0 and F > 0: refused (observed, xf0 and out_vel may be null)\n");

  {
    void* q[8];
    for (int j = 0; j < 8; ++j) q[j] = p[j];
    q[5] = (char*)work8.data() + 4;
    expect(call(q, L, F, S, good, 0, false), MMMOT_EINVAL, "work not 8-byte aligned");
  }
  for (int s : {0, -1, INT_MIN}) expect(call(p, L, F, s, good, 0, false), MMMOT_EINVAL, "S < 1");
  expect(call(p, -1, F, S, good, 0, false), MMMOT_EINVAL, "L < 0");
  expect(call(p, INT_MIN, F, S, good, 0, false), MMMOT_EINVAL, "L = INT_MIN");
  expect(call(p, L, -1, S, good, 0, false), MMMOT_EINVAL, "F < 0");
  expect(call(p, INT_MAX, F, S, good, 0, false), MMMOT_EINVAL, "a scratch index past 32 bits");
  expect(call(p, INT_MAX / 75 + 1, F, S, good, 0, false), MMMOT_EINVAL, "the first L whose scratch passes 32 bits");
  for (int flip : {2, -1, INT_MAX}) expect(call(p, L, F, S, good, flip, false), MMMOT_EINVAL, "yaw_flip outside {0, 1}");
  std::printf("S < 1, negative sizes, L beyond the scratch index, a misaligned work, a bad yaw_flip: refused\n");

  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  for (int i = 0; i < 8; ++i)
    for (double v : {-1.0, -1e-300, nan, inf, -inf}) {
      double prm[8];
      for (int j = 0; j < 8; ++j) prm[j] = j == i ? v : good[j];
      expect(call(p, L, F, S, prm, 0, true), MMMOT_EINVAL, "a negative, NaN or infinite parameter");
      expect(call(p, 0, F, S, prm, 0, true), MMMOT_EINVAL, "a bad parameter with L = 0");
    }
  for (int i : {2, 5}) {
    double prm[8];
    for (int j = 0; j < 8; ++j) prm[j] = j == i ? 0.0 : good[j];
    expect(call(p, L, F, S, prm, 0, false), MMMOT_EINVAL, "v0 = 0 for a group with r > 0");
  }
  std::printf("negative, NaN and infinite parameters, v0 <= 0 with r > 0: refused\n");

  void* none[8] = {};
  expect(call(none, 0, F, S, good, 0, false), MMMOT_OK, "L = 0, nulls");
  expect(call(none, L, 0, S, good, 1, false), MMMOT_OK, "F = 0, nulls");
  expect(call(p, 0, 0, S, good, 0, true), MMMOT_OK, "L = F = 0");
  expect(call(none, 0, 0, 0, good, 0, false), MMMOT_EINVAL, "L = 0, S = 0");
  std::printf("L = 0 or F = 0: a no-op that returns 0\n");

  std::printf(failures ? "%d wrong answers\n" : "all argument checks answered as documented (%d wrong)\n", failures);
  return failures ? 1 : 0;
}
