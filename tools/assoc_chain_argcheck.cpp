// Stand-alone host program for a sanitizer run of the argument-checking host side of mmmot_associate_chains and
// mmmot_set_chain_variant (mmmot_amd/csrc/assign_chain.hip).  CPU only: every call below is answered before any launch,
// so it needs no GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined mmmot_amd/csrc/assign_chain.hip tools/assoc_chain_argcheck.cpp \
//       -fsanitize=address,undefined -o /tmp/assoc_chain_argcheck && /tmp/assoc_chain_argcheck
//
// The chain table is device memory to the entry point: its entries are checked by the kernel (a chain outside the limits
// gets a NaN objective) and, on the host, by torch_ops.chain_layout.  What the entry point itself answers is the pointers
// and the launch sizes; the tables below - null, and filled with values no chain may have - stand in for device pointers
// and must never be read through.
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
  std::vector<float> sc(8, 1.f), lk(16, 1.f), out(64, 0.f);
  std::vector<int> off = {0};
  std::vector<double> obj(1, 0.0);
  // tables no chain may have: T = 1, T = 9, a frame of 513, negative offsets, INT_MAX everywhere
  std::vector<std::vector<int>> tables = {
      {1, 0, 0, 4, 0, 0, 0, 0, 0, 0, 0},           {9, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1},
      {2, 0, 0, 513, 1, 0, 0, 0, 0, 0, 0},         {2, -1, -1, 2, 2, 0, 0, 0, 0, 0, 0},
      std::vector<int>(MMMOT_CHAIN_ROW, INT_MAX),  std::vector<int>(MMMOT_CHAIN_ROW, INT_MIN)};
  const float* s = sc.data();
  const float* l = lk.data();
  float* o = out.data();
  const int* oo = off.data();
  double* ob = obj.data();
  const int* good = tables[3].data();

  expect(mmmot_associate_chains(nullptr, s, s, l, good, 1, 2, 4, o, oo, ob, nullptr), MMMOT_EINVAL, "null det");
  expect(mmmot_associate_chains(s, nullptr, s, l, good, 1, 2, 4, o, oo, ob, nullptr), MMMOT_EINVAL, "null new");
  expect(mmmot_associate_chains(s, s, nullptr, l, good, 1, 2, 4, o, oo, ob, nullptr), MMMOT_EINVAL, "null end");
  expect(mmmot_associate_chains(s, s, s, nullptr, good, 1, 2, 4, o, oo, ob, nullptr), MMMOT_EINVAL, "null link");
  expect(mmmot_associate_chains(s, s, s, l, nullptr, 1, 2, 4, o, oo, ob, nullptr), MMMOT_EINVAL, "null chains");
  expect(mmmot_associate_chains(s, s, s, l, good, 1, 2, 4, nullptr, oo, ob, nullptr), MMMOT_EINVAL, "null out");
  expect(mmmot_associate_chains(s, s, s, l, good, 1, 2, 4, o, nullptr, ob, nullptr), MMMOT_EINVAL, "null out_off");
  expect(mmmot_associate_chains(s, s, s, l, good, 1, 2, 4, o, oo, nullptr, nullptr), MMMOT_EINVAL, "null objective");
  std::printf("null pointers, the chain table among them: refused\n");

  // invalid launch sizes, with every invalid table in turn: refused before the table could matter
  for (const auto& t : tables) {
    for (int B : {0, -1, INT_MIN})
      expect(mmmot_associate_chains(s, s, s, l, t.data(), B, 2, 4, o, oo, ob, nullptr), MMMOT_EINVAL, "B < 1");
    for (int n : {0, -1, 513, INT_MAX, INT_MIN})
      expect(mmmot_associate_chains(s, s, s, l, t.data(), 1, n, 4, o, oo, ob, nullptr), MMMOT_EINVAL, "max_n outside [1, 512]");
    for (int L : {0, -1, 1, 1025, INT_MAX, INT_MIN})
      expect(mmmot_associate_chains(s, s, s, l, t.data(), 1, 2, L, o, oo, ob, nullptr), MMMOT_EINVAL,
             "max_L outside [max_n, 1024]");
    expect(mmmot_associate_chains(s, s, s, l, t.data(), 1, 2, 17, o, oo, ob, nullptr), MMMOT_EINVAL, "max_L > 8 max_n");
    expect(mmmot_associate_chains(s, s, s, l, t.data(), 1, 100, 801, o, oo, ob, nullptr), MMMOT_EINVAL, "max_L > 8 max_n");
  }
  std::printf("B < 1, max_n outside [1, 512], max_L outside [max_n, min(1024, 8 max_n)]: refused, whatever the table\n");

  for (int v : {-1, 3, INT_MAX, INT_MIN}) expect(mmmot_set_chain_variant(v), MMMOT_EINVAL, "variant outside [0, 2]");
  for (int v : {1, 2, 0}) expect(mmmot_set_chain_variant(v), MMMOT_OK, "variant in [0, 2]");
  std::printf("variant setter: [0, 2] accepted, the rest refused\n");

  std::printf(failures ? "%d wrong answers\n" : "all argument checks answered as documented (%d wrong)\n", failures);
  return failures ? 1 : 0;
}
