// Host reference of the CU scan (include/gm_cuscan_sig.h) under ASan/UBSan: every test at the
// iteration counts the Python tests use, with properties that need no second implementation.
// No GPU, no HIP, nothing loaded into an interpreter; part of `make -C native check`.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <set>
#include <vector>

#include "gm_cuscan_sig.h"

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static std::vector<uint32_t> table(uint32_t test, uint64_t seed, uint32_t iters) {
  std::vector<uint32_t> out(GM_CUSCAN_SIG_WORDS, 0xDEADBEEFu);
  gm_cuscan_expected_host(test, seed, iters, out.data());
  return out;
}

int main() {
  const uint64_t seeds[2] = {0, 0x0123456789ABCDEFull};
  const uint32_t iters[3] = {1, 3, GM_CUSCAN_DEFAULT_ITERS};
  const uint32_t tests[4] = {GM_CUSCAN_VALU_INT, GM_CUSCAN_VALU_F32, GM_CUSCAN_MFMA, GM_CUSCAN_LDS};
  for (uint64_t seed : seeds)
    for (uint32_t it : iters)
      for (uint32_t test : tests) {
        const std::vector<uint32_t> a = table(test, seed, it), b = table(test, seed, it);
        EXPECT(a == b);                                        // a pure function
        EXPECT(a != table(test, seed ^ 1, it));                // of the seed
        EXPECT(a != table(test, seed, it + 1));                // and of iters
        if (test == GM_CUSCAN_VALU_F32) {
          std::set<uint32_t> distinct(a.begin(), a.end());
          EXPECT(distinct.size() >= 1000);
          for (uint32_t w : a) {
            float f;
            memcpy(&f, &w, 4);
            EXPECT(f >= 1.0f && f < 2.0f);
          }
        }
        if (test == GM_CUSCAN_MFMA) {
          for (uint32_t w : a) {
            float f;
            memcpy(&f, &w, 4);
            EXPECT(f == floorf(f) && fabsf(f) <= 32.0f * 16.0f * it * GM_CUSCAN_MFMA_STEPS);
          }
        }
        if (test == GM_CUSCAN_LDS)
          for (uint32_t t = 0; t < GM_CUSCAN_THREADS; ++t) EXPECT(a[4 * t + 3] == 0);
      }

  // the MFMA bound itself: the largest accepted step count keeps every sum below 2^24
  EXPECT(32ull * 16 * GM_CUSCAN_MFMA_STEPS * GM_CUSCAN_MFMA_MAX_ITERS < (1ull << 24));
  EXPECT(32ull * 16 * GM_CUSCAN_MFMA_STEPS * (GM_CUSCAN_MFMA_MAX_ITERS + 1) >= (1ull << 24));
  for (int j = 0; j < 8; ++j)
    for (uint32_t n = 0; n < 16; ++n) {
      const int32_t e = gm_cuscan_mfma_entry(n << (4 * j), j);
      EXPECT(e >= -4 && e <= 4);
    }

  // the LDS permutation reaches every address exactly once, and every thread reads words that
  // another wave wrote (phase 1 writes word a from thread (a / 4) % 256)
  std::vector<int> hit(GM_CUSCAN_LDS_WORDS, 0);
  std::vector<int> cross(GM_CUSCAN_THREADS, 0);
  for (uint32_t j = 0; j < GM_CUSCAN_LDS_WORDS; ++j) {
    const uint32_t a = gm_cuscan_lds_perm(j);
    EXPECT(a < GM_CUSCAN_LDS_WORDS);
    if (a < GM_CUSCAN_LDS_WORDS) ++hit[a];
    cross[j & 255] += (((a >> 2) & 255) >> 6) != ((j & 255) >> 6);
  }
  for (int h : hit) EXPECT(h == 1);
  long crossing = 0;
  for (int c : cross) {
    EXPECT(c > 0);
    crossing += c;
  }
  EXPECT(crossing * 10 >= (long)GM_CUSCAN_LDS_WORDS * 7);      // about three in four
  std::vector<int> hit4(GM_CUSCAN_LDS_WORDS / 4, 0);
  for (uint32_t t = 0; t < GM_CUSCAN_THREADS; ++t)
    for (uint32_t k = 0; k < GM_CUSCAN_LDS_WORDS / 1024; ++k) {
      const uint32_t v = gm_cuscan_lds_vec(t, k);
      EXPECT(v < GM_CUSCAN_LDS_WORDS / 4);
      if (v < GM_CUSCAN_LDS_WORDS / 4) ++hit4[v];
      EXPECT(((v & 255) >> 6) != (t >> 6));
    }
  for (int h : hit4) EXPECT(h == 1);

  if (failures) {
    printf("%d failure(s)\n", failures);
    return 1;
  }
  printf("test_cuscan_host: ok\n");
  return 0;
}
