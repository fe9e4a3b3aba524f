// Stand-alone host program for a sanitizer run of the argument-checking host side of mmmot_align_points
// (mmmot_amd/csrc/align_points.hip).  CPU only: every call below is answered before any launch, so it needs no GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined mmmot_amd/csrc/align_points.hip tools/align_points_argcheck.cpp \
//       -fsanitize=address,undefined -o /tmp/align_points_argcheck && /tmp/align_points_argcheck
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
  std::vector<float> pts(4 * 4, 1.f), out(4 * 4, 0.f);
  std::vector<int> seg = {0, 4};
  std::vector<double> xf(MMMOT_ALIGN_REC, 0.0);
  const float* p = pts.data();
  float* o = out.data();
  const int* s = seg.data();
  const double* x = xf.data();

  for (int F : {-1, 0, 1, 2, 5, 8, INT_MAX, INT_MIN})
    expect(mmmot_align_points(p, F, 4, 1, s, x, 1, o, 0, 4, nullptr), MMMOT_EINVAL, "F outside {3, 4}");
  std::printf("F outside {3, 4}: refused\n");

  expect(mmmot_align_points(nullptr, 3, 4, 1, s, x, 1, o, 0, 3, nullptr), MMMOT_EINVAL, "null pts");
  expect(mmmot_align_points(p, 3, 4, 1, nullptr, x, 1, o, 0, 3, nullptr), MMMOT_EINVAL, "null seg_row0");
  expect(mmmot_align_points(p, 3, 4, 1, s, nullptr, 1, o, 0, 3, nullptr), MMMOT_EINVAL, "null xf");
  expect(mmmot_align_points(p, 3, 4, 1, s, x, 1, nullptr, 0, 3, nullptr), MMMOT_EINVAL, "null out");
  std::printf("null pointers with Q > 0: refused\n");

  for (int chain : {-1, 5, 6, INT_MAX, INT_MIN})
    expect(mmmot_align_points(p, 3, 4, 1, s, x, chain, o, 0, 3, nullptr), MMMOT_EINVAL, "chain outside [0, 4]");
  std::printf("chain outside [0, 4]: refused\n");

  expect(mmmot_align_points(p, 3, -1, 1, s, x, 1, o, 0, 3, nullptr), MMMOT_EINVAL, "Q < 0");
  expect(mmmot_align_points(p, 3, INT_MIN, 1, s, x, 1, o, 0, 3, nullptr), MMMOT_EINVAL, "Q = INT_MIN");
  expect(mmmot_align_points(p, 3, 4, -1, s, x, 1, o, 0, 3, nullptr), MMMOT_EINVAL, "NS < 0");
  expect(mmmot_align_points(p, 3, 4, 0, s, x, 1, o, 0, 3, nullptr), MMMOT_EINVAL, "NS = 0 with Q > 0");
  expect(mmmot_align_points(p, 3, 4, 1, s, x, 1, o, -1, 3, nullptr), MMMOT_EINVAL, "out_row0 < 0");
  expect(mmmot_align_points(p, 3, 4, 1, s, x, 1, o, LONG_MIN, 3, nullptr), MMMOT_EINVAL, "out_row0 = LONG_MIN");
  expect(mmmot_align_points(p, 4, 4, 1, s, x, 1, o, 0, 3, nullptr), MMMOT_EINVAL, "ldo < F");
  expect(mmmot_align_points(p, 3, 4, 1, s, x, 1, o, 0, -3, nullptr), MMMOT_EINVAL, "ldo < 0");
  std::printf("negative sizes, rows without a segment, overlapping rows: refused\n");

  expect(mmmot_align_points(nullptr, 3, 0, 0, nullptr, nullptr, 1, nullptr, 0, 3, nullptr), MMMOT_OK, "Q = 0, nulls");
  expect(mmmot_align_points(p, 4, 0, 1, s, x, 4, o, 7, 4, nullptr), MMMOT_OK, "Q = 0");
  expect(mmmot_align_points(p, 4, 0, 1, s, x, 0, o, LONG_MAX, 0, nullptr), MMMOT_OK, "Q = 0, extreme offset");
  expect(mmmot_align_points(nullptr, 2, 0, 0, nullptr, nullptr, 1, nullptr, 0, 3, nullptr), MMMOT_EINVAL, "Q = 0, bad F");
  std::printf("Q = 0: a no-op that returns 0\n");

  std::printf(failures ? "%d wrong answers\n" : "all argument checks answered as documented (%d wrong)\n", failures);
  return failures ? 1 : 0;
}
