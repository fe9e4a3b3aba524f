// Runs mmmot_crop_augment's kernel on the host (common.h of this directory) over the cases of a file written by
// tests/test_augment_host_cpu.py: per case L, S, crops, table, expected bytes, expected floats.  Buffers are allocated to
// their exact size, so the sanitizer reports any access past either end.  Exit status 0: every output equal.
#include "crop_augment.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static size_t rd(void* p, size_t size, size_t n, FILE* f) { return fread(p, size, n, f) == n ? n : (exit(2), 0); }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const float ms[6] = {0.485f, 0.456f, 0.406f, 0.229f, 0.224f, 0.225f};
  int ncase, bad = 0;
  rd(&ncase, 4, 1, f);
  for (int ci = 0; ci < ncase; ++ci) {
    int L, S, check;
    rd(&L, 4, 1, f);
    rd(&S, 4, 1, f);
    rd(&check, 4, 1, f);  // 0: an out-of-range table - only the accesses are looked at
    const size_t nb = (size_t)L * S * S * 3;
    std::vector<unsigned char> crops(nb), want8(nb);
    std::vector<int> par((size_t)L * 5);
    std::vector<float> wantf(nb);
    rd(crops.data(), 1, nb, f);
    rd(par.data(), 4, (size_t)L * 5, f);
    rd(want8.data(), 1, nb, f);
    rd(wantf.data(), 4, nb, f);
    for (int mode = 0; mode < 4; ++mode) {  // fp32 alone, bytes alone, both, both from an input pointer off by one byte
      const int mis = mode == 3;
      unsigned char* in = (unsigned char*)malloc(nb + mis);
      memcpy(in + mis, crops.data(), nb);
      float* o = mode != 1 ? (float*)malloc(nb * 4) : nullptr;
      unsigned char* o8 = mode != 0 ? (unsigned char*)malloc(nb) : nullptr;
      const int st = mmmot_crop_augment(in + mis, par.data(), L, S, ms, o, o8, nullptr);
      size_t d8 = 0, df = 0;
      if (check && o8) d8 = memcmp(o8, want8.data(), nb) != 0;
      if (check && o) df = memcmp(o, wantf.data(), nb * 4) != 0;
      if (st || d8 || df) {
        printf("case %d (L=%d S=%d) mode %d: status %d, bytes differ %zu, floats differ %zu\n", ci, L, S, mode, st, d8, df);
        ++bad;
      }
      free(in);
      free(o);
      free(o8);
    }
  }
  fclose(f);
  printf("%d cases, %d bad\n", ncase, bad);
  return bad != 0;
}
