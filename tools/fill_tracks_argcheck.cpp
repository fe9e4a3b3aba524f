// Stand-alone host program for a sanitizer run of the argument-checking host side of mmmot_fill_tracks
// (mmmot_amd/csrc/fill_tracks.hip).  CPU only: every call below is answered before any launch, so it needs no GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined mmmot_amd/csrc/fill_tracks.hip tools/fill_tracks_argcheck.cpp \
//       -fsanitize=address,undefined -o /tmp/fill_tracks_argcheck && /tmp/fill_tracks_argcheck
//
// Prints one line per group and returns non-zero on the first wrong answer; the sanitizers abort on their own findings.
#include <climits>
#include <cstdio>
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
  const int L = 2, F = 3, S = 1, cap = 1;
  std::vector<float> det(L * 12, 1.f), out(cap * 12, 0.f);
  std::vector<int> ids = {1, 1}, fs = {0, 1, 1, 2}, no = {0, 1, 2}, ss = {0, 3};
  std::vector<int> work(MMMOT_FILL_WORK(L)), fill(F + 1), oid(cap), osrc(2 * cap), info(4 * S);
  std::vector<double> wtab((MMMOT_FILL_MAX + 2) * (MMMOT_FILL_MAX + 2), 0.0);
  void* p[12] = {det.data(), ids.data(), fs.data(), no.data(), ss.data(), wtab.data(),
                 work.data(), fill.data(), out.data(), oid.data(), osrc.data(), info.data()};
  auto call = [&](void** q, int l, int f, int s, int max_fill, int capacity) {
    return mmmot_fill_tracks((const float*)q[0], (const int*)q[1], (const int*)q[2], (const int*)q[3], (const int*)q[4],
                             nullptr, (const double*)q[5], l, f, s, max_fill, capacity, (int*)q[6], (int*)q[7],
                             (float*)q[8], (int*)q[9], (int*)q[10], (int*)q[11], nullptr);
  };

  for (int i = 0; i < 12; ++i) {
    void* q[12];
    for (int j = 0; j < 12; ++j) q[j] = j == i ? nullptr : p[j];
    expect(call(q, L, F, S, 7, cap), MMMOT_EINVAL, "a null pointer");
  }
  std::printf("null pointers with L > 0 and F > 0: refused\n");

  for (int m : {0, -1, 31, 32, INT_MAX, INT_MIN}) expect(call(p, L, F, S, m, cap), MMMOT_EINVAL, "max_fill outside [1, 30]");
  std::printf("max_fill outside [1, 30]: refused\n");

  for (int s : {0, -1, INT_MIN}) expect(call(p, L, F, s, 7, cap), MMMOT_EINVAL, "S < 1");
  expect(call(p, -1, F, S, 7, cap), MMMOT_EINVAL, "L < 0");
  expect(call(p, INT_MIN, F, S, 7, cap), MMMOT_EINVAL, "L = INT_MIN");
  expect(call(p, L, -1, S, 7, cap), MMMOT_EINVAL, "F < 0");
  expect(call(p, L, F, S, 7, -1), MMMOT_EINVAL, "capacity < 0");
  expect(call(p, INT_MAX, F, S, 7, cap), MMMOT_EINVAL, "a scratch index past 32 bits");
  std::printf("S < 1, negative sizes, L beyond the scratch index: refused\n");

  void* none[12] = {};
  expect(call(none, 0, F, S, 7, 0), MMMOT_OK, "L = 0, nulls");
  expect(call(none, L, 0, S, 30, INT_MAX), MMMOT_OK, "F = 0, nulls");
  expect(call(p, 0, 0, S, 1, cap), MMMOT_OK, "L = F = 0");
  expect(call(none, 0, 0, 0, 7, 0), MMMOT_EINVAL, "L = 0, S = 0");
  expect(call(none, 0, 0, S, 0, 0), MMMOT_EINVAL, "L = 0, bad max_fill");
  std::printf("L = 0 or F = 0: a no-op that returns 0\n");

  std::printf(failures ? "%d wrong answers\n" : "all argument checks answered as documented (%d wrong)\n", failures);
  return failures ? 1 : 0;
}
