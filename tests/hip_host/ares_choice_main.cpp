// Stand-alone host program for tests/test_ares_choice_cpu.py: asks mmmot_ares_choose (csrc/ares_choice.h), the one
// function that picks the kernel behind mmmot_gemm_ares, for each case of a text file and prints the kernel's name.
//   line in : K N mode variant n_cu T ldx ldsc ldosc lddb      (lddb = 0: no dbias rows)
//   line out: refuse | streaming | weight-resident | independent-wave | weights-in-registers
#include <cstdio>

#include "../../include/mmmot_hip.h"
#include "../../mmmot_amd/csrc/ares_choice.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  static const char* const names[] = {"refuse", "streaming", "weight-resident", "independent-wave", "weights-in-registers"};
  static const float some_rows[4] = {0.f, 0.f, 0.f, 0.f};  // the chooser asks whether dbias is there, never reads it
  int K, N, mode, variant, n_cu, T, ldx, ldsc, ldosc, lddb;
  while (fscanf(f, "%d %d %d %d %d %d %d %d %d %d", &K, &N, &mode, &variant, &n_cu, &T, &ldx, &ldsc, &ldosc, &lddb) == 10) {
    mmmot_gemm_ares_args a = {};
    a.K = K;
    a.N = N;
    a.T = T;
    a.ldx = ldx;
    a.ldsc = ldsc;
    a.ldosc = ldosc;
    a.lddb = lddb;
    a.dbias = lddb ? some_rows : nullptr;
    const int which = (int)mmmot_ares_choose(&a, mode, n_cu, variant);
    if (which < 0 || which > 4) return 3;
    puts(names[which]);
  }
  fclose(f);
  return 0;
}
