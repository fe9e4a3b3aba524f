// Stand-alone host program for a sanitizer run of the host side of csrc/adam_step.hip: the argument checks of
// mmmot_adam_step and the host-side chunk-table builder mmmot_adam_chunks.  CPU only: every mmmot_adam_step call below is
// answered before any launch and mmmot_adam_chunks never touches a device, so it needs no GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined mmmot_amd/csrc/adam_step.hip tools/adam_step_argcheck.cpp \
//       -fsanitize=address,undefined -o /tmp/adam_step_argcheck && /tmp/adam_step_argcheck
//
// The chunk tables are sized EXACTLY (a std::vector of 2 * count ints), so a row written past the count is a heap
// overflow the sanitizer reports.  Prints one line per group and returns non-zero on the first wrong answer; the
// sanitizers abort on their own findings.
#include <climits>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../include/mmmot_hip.h"

static int failures = 0;

static void expect(long long got, long long want, const char* what) {
  if (got != want) {
    std::printf("FAIL %s: got %lld, expected %lld\n", what, got, want);
    ++failures;
  }
}

int main() {
  static_assert(sizeof(mmmot_adam_row) == 64, "row layout");
  // real host arrays stand in for the device tables: the checks never read through them
  std::vector<mmmot_adam_row> rows(2);
  std::vector<int> chunks = {0, 0, 1, 0};
  const mmmot_adam_row* t = rows.data();
  const int* c = chunks.data();
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

  expect(mmmot_adam_step(nullptr, 2, c, 2, 0.9, 0.99, 1e-8, nullptr), MMMOT_EINVAL, "null tensor table");
  expect(mmmot_adam_step(t, 2, nullptr, 2, 0.9, 0.99, 1e-8, nullptr), MMMOT_EINVAL, "null chunk table");
  expect(mmmot_adam_step(nullptr, 0, nullptr, 0, 0.9, 0.99, 1e-8, nullptr), MMMOT_EINVAL, "null tables, no work");
  std::printf("null tables: refused\n");

  for (int n : {0, -1, INT_MIN}) {
    expect(mmmot_adam_step(t, n, c, 2, 0.9, 0.99, 1e-8, nullptr), MMMOT_EINVAL, "n_tensors < 1");
    expect(mmmot_adam_step(t, 2, c, n, 0.9, 0.99, 1e-8, nullptr), MMMOT_EINVAL, "n_chunks < 1");
  }
  std::printf("zero and negative counts with non-null work: refused\n");

  for (double b : {-0.1, -inf, 1.0, 1.0000001, 2.0, inf, nan}) {
    expect(mmmot_adam_step(t, 2, c, 2, b, 0.99, 1e-8, nullptr), MMMOT_EINVAL, "beta1 outside [0, 1)");
    expect(mmmot_adam_step(t, 2, c, 2, 0.9, b, 1e-8, nullptr), MMMOT_EINVAL, "beta2 outside [0, 1)");
  }
  for (double e : {-1e-30, -1.0, -inf, nan, inf})
    expect(mmmot_adam_step(t, 2, c, 2, 0.9, 0.99, e, nullptr), MMMOT_EINVAL, "eps < 0 or not finite");
  std::printf("betas outside [0, 1), eps < 0, NaN: refused\n");

  expect(mmmot_adam_step((const mmmot_adam_row*)((const char*)t + 4), 1, c, 2, 0.9, 0.99, 1e-8, nullptr), MMMOT_EINVAL,
         "misaligned tensor table");
  expect(mmmot_adam_step(t, 2, (const int*)((const char*)c + 2), 1, 0.9, 0.99, 1e-8, nullptr), MMMOT_EINVAL,
         "misaligned chunk table");
  std::printf("misaligned tables: refused\n");

  // ---- the chunk table ------------------------------------------------------------------------------------------------
  const long long C = mmmot_adam_chunk_elems();
  expect(C, MMMOT_ADAM_CHUNK, "mmmot_adam_chunk_elems");
  const std::vector<long long> numel = {1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3, 2359296};
  long long count = -7;
  expect(mmmot_adam_chunks(numel.data(), (int)numel.size(), nullptr, 0, &count), MMMOT_OK, "count alone");
  long long want = 0;
  for (long long n : numel) want += (n + C - 1) / C;
  expect(count, want, "chunk count");
  std::vector<int> table(2 * (size_t)count, -1);
  long long count2 = 0;
  expect(mmmot_adam_chunks(numel.data(), (int)numel.size(), table.data(), count, &count2), MMMOT_OK, "chunk table");
  expect(count2, count, "count of the second call");
  {
    // every element of every tensor is covered by exactly one row, rows in tensor order
    long long w = 0;
    for (size_t i = 0; i < numel.size(); ++i)
      for (long long k = 0; k * C < numel[i]; ++k, ++w) {
        expect(table[2 * w], (long long)i, "row: tensor index");
        expect(table[2 * w + 1], k, "row: chunk index");
      }
    expect(w, count, "rows walked");
  }
  std::printf("chunk table of %zu tensors: %lld rows, every element covered once\n", numel.size(), count);

  std::vector<int> small(2 * (size_t)(count - 1), -1);
  expect(mmmot_adam_chunks(numel.data(), (int)numel.size(), small.data(), count - 1, &count2), MMMOT_EINVAL, "cap too small");
  for (int v : small) expect(v, -1, "nothing written when cap is too small");
  expect(mmmot_adam_chunks(nullptr, 1, table.data(), count, &count2), MMMOT_EINVAL, "null h_numel");
  expect(mmmot_adam_chunks(numel.data(), 1, table.data(), count, nullptr), MMMOT_EINVAL, "null h_count");
  expect(mmmot_adam_chunks(numel.data(), 0, table.data(), count, &count2), MMMOT_EINVAL, "n_tensors = 0");
  expect(mmmot_adam_chunks(numel.data(), -3, table.data(), count, &count2), MMMOT_EINVAL, "n_tensors < 0");
  expect(mmmot_adam_chunks(numel.data(), 1, nullptr, 5, &count2), MMMOT_EINVAL, "cap > 0 without a table");
  expect(mmmot_adam_chunks(numel.data(), 1, table.data(), -1, &count2), MMMOT_EINVAL, "cap < 0");
  for (long long bad : {0LL, -1LL, LLONG_MIN}) {
    const std::vector<long long> n2 = {8, bad};
    expect(mmmot_adam_chunks(n2.data(), 2, table.data(), count, &count2), MMMOT_EINVAL, "numel < 1");
  }
  {
    const std::vector<long long> huge = {LLONG_MAX, LLONG_MAX};  // more rows than a grid holds: refused, no overflow
    expect(mmmot_adam_chunks(huge.data(), 2, nullptr, 0, &count2), MMMOT_EINVAL, "more than 2^31 - 1 rows");
    const std::vector<long long> edge = {(long long)INT_MAX * C, 1};
    expect(mmmot_adam_chunks(edge.data(), 1, nullptr, 0, &count2), MMMOT_OK, "exactly 2^31 - 1 rows");
    expect(count2, INT_MAX, "count at the limit");
    expect(mmmot_adam_chunks(edge.data(), 2, nullptr, 0, &count2), MMMOT_EINVAL, "one row past the limit");
  }
  std::printf("short tables, null pointers, sizes < 1, more rows than a grid holds: refused\n");

  std::printf(failures ? "%d wrong answers\n" : "all argument checks answered as documented (%d wrong)\n", failures);
  return failures ? 1 : 0;
}
