// The liveness probe's expected table and verdict (include/gm_quick_ref.h) under ASan/UBSan: the
// table against a second, naive evaluation written here, and the verdict over every single-bit
// flip of every word. No GPU, no HIP, nothing loaded into an interpreter; part of
// `make -C native check`.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "gm_quick_ref.h"

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                 \
    }                                                             \
  } while (0)

// the formula of gm_probe.h in 64-bit arithmetic, reduced only at the end
static void naive(uint32_t salt, uint32_t out[66]) {
  uint64_t sum = 0;
  for (uint64_t l = 0; l < 64; ++l) {
    const uint64_t v = ((l * 2654435761ull) & 0xFFFFFFFFull) ^ salt;
    out[l] = (uint32_t)v;
    sum += v;
  }
  out[64] = (uint32_t)(sum & 0xFFFFFFFFull);
  out[65] = 64;
}

static uint32_t check_of(uint32_t word) {
  return word < 64 ? GM_QUICK_BAD_LANES : word == 64 ? GM_QUICK_BAD_SUM : GM_QUICK_BAD_BALLOT;
}

int main() {
  static_assert(GM_QUICK_WORDS == 66 && GM_QUICK_SUM_WORD == 64 && GM_QUICK_BALLOT_WORD == 65, "");
  const uint32_t salts[] = {0u, 1u, 0x9e3779b9u, 0x9e3779b9u ^ 7u, 0xFFFFFFFFu, 0x80000000u};
  for (uint32_t salt : salts) {
    uint32_t want[66], got[66 + 2];
    naive(salt, want);
    got[0] = got[67] = 0xDEADBEEFu;  // the table writes 66 words and no more
    gm_quick_expected(salt, got + 1);
    EXPECT(memcmp(got + 1, want, sizeof(want)) == 0);
    EXPECT(got[0] == 0xDEADBEEFu && got[67] == 0xDEADBEEFu);
    for (uint32_t l = 0; l < 64; ++l) EXPECT(gm_quick_lane_value(l, salt) == want[l]);

    EXPECT(gm_quick_verdict(want, salt) == 0);
    // every single-bit flip fails, and names the flipped word's check alone
    uint32_t w[66];
    for (uint32_t word = 0; word < 66; ++word)
      for (uint32_t bit = 0; bit < 32; ++bit) {
        memcpy(w, want, sizeof(w));
        w[word] ^= 1u << bit;
        EXPECT(gm_quick_verdict(w, salt) == check_of(word));
      }
    // a wave32 machine: everything right but the ballot count
    memcpy(w, want, sizeof(w));
    w[65] = 32;
    EXPECT(gm_quick_verdict(w, salt) == GM_QUICK_BAD_BALLOT);
    // all three at once
    w[64] += 1;
    w[63] = ~w[63];
    EXPECT(gm_quick_verdict(w, salt) ==
           (GM_QUICK_BAD_LANES | GM_QUICK_BAD_SUM | GM_QUICK_BAD_BALLOT));
    // another salt's table: every lane word differs; the sum of 64 equal XORs need not
    naive(salt ^ 0x10u, w);
    EXPECT(gm_quick_verdict(w, salt) & GM_QUICK_BAD_LANES);
    EXPECT(gm_quick_verdict(w, salt ^ 0x10u) == 0);
  }
  EXPECT(gm_quick_salt(0) == 0x9e3779b9u && gm_quick_salt(5) == (0x9e3779b9u ^ 5u));

  if (failures) {
    printf("%d failure(s)\n", failures);
    return 1;
  }
  printf("test_quick_host: ok\n");
  return 0;
}
