// Host fill and compare of the host-link test (include/gm_hostlink_host.h) under ASan/UBSan,
// word by word against gm_memtest_expected. No GPU, no HIP, nothing loaded into an interpreter;
// part of `make -C native check`.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "gm_hostlink_host.h"

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static const uint32_t kPatterns[5] = {GM_MEMTEST_ADDR, GM_MEMTEST_SOLID, GM_MEMTEST_CHECKER,
                                      GM_MEMTEST_WALK, GM_MEMTEST_RANDOM};
static const uint64_t kSeed = 0x243F6A8885A308D3ull;

// fill + compare of `bytes` at `base`, with guard words around the buffer
static void fill_and_compare(uint64_t bytes, uint64_t base) {
  const uint64_t n = bytes / 8, guard = 0xFEEDFACECAFEBEEFull;
  for (uint32_t p : kPatterns)
    for (int invert = 0; invert < 2; ++invert) {
      std::vector<uint64_t> buf(n + 2, guard);
      gm_hl_host_fill(buf.data() + 1, n, p, invert, kSeed, 3, base);
      EXPECT(buf[0] == guard && buf[n + 1] == guard);
      bool same = true;
      for (uint64_t i = 0; i < n; ++i) {
        const uint64_t e = gm_memtest_expected(p, kSeed, 3, base + 8 * i);
        same &= buf[1 + i] == (invert ? ~e : e);
      }
      EXPECT(same);
      gm_hl_host_cmp_t c;
      memset(&c, 0xFF, sizeof(c));
      gm_hl_host_compare(buf.data() + 1, n, p, invert, kSeed, 3, base, &c);
      EXPECT(c.words == 0 && c.bits == 0 && c.stuck == 0 && c.records_filled == 0);
      // the other polarity differs in every bit of every word
      gm_hl_host_compare(buf.data() + 1, n, p, !invert, kSeed, 3, base, &c);
      EXPECT(c.words == n && c.bits == 64 * n && c.stuck == ~0ull);
      EXPECT(c.records_filled == (n < 16 ? n : 16));
      for (uint32_t i = 0; i < c.records_filled; ++i) {
        EXPECT(c.offset[i] == base + 8 * i);
        EXPECT((c.expected[i] ^ c.got[i]) == ~0ull);
      }
    }
}

int main() {
  // 16 bytes, 4080, an odd multiple of 16, and a base offset that crosses 2^35
  const uint64_t sizes[3] = {16, 4080, 16 * 1237};
  const uint64_t bases[3] = {0, 4096, (1ull << 35) - 2048};
  for (uint64_t s : sizes)
    for (uint64_t b : bases) fill_and_compare(s, b);
  {
    // the pattern really changes across 2^35: the words on both sides are their own offsets
    uint64_t w[2];
    gm_hl_host_fill(w, 2, GM_MEMTEST_ADDR, 0, 0, 0, (1ull << 35) - 8);
    EXPECT(w[0] == (1ull << 35) - 8 && w[1] == (1ull << 35));
  }

  // planted flips: offsets, counts, bit errors, stuck mask, ascending records; large enough
  // for the threaded split (4 threads from 4 Mi words)
  const uint64_t n = 4 * GM_HL_HOST_WORDS_PER_THREAD + 3;
  EXPECT(gm_hl_host_threads(n) == 4);
  EXPECT(gm_hl_host_threads(1) == 1);
  EXPECT(gm_hl_host_threads(2 * GM_HL_HOST_WORDS_PER_THREAD) == 2);
  EXPECT(gm_hl_host_threads(1ull << 40) == GM_HL_HOST_MAX_THREADS);
  {
    const uint64_t base = (1ull << 35) - 8 * (n / 2);
    std::vector<uint64_t> buf(n);
    gm_hl_host_fill(buf.data(), n, GM_MEMTEST_RANDOM, 0, kSeed, 1, base);
    bool same = true;
    for (uint64_t i = 0; i < n; ++i)
      same &= buf[i] == gm_memtest_expected(GM_MEMTEST_RANDOM, kSeed, 1, base + 8 * i);
    EXPECT(same);
    // first word, last word, one in each thread's part, two neighbours
    const uint64_t at[6] = {0, 12345, GM_HL_HOST_WORDS_PER_THREAD + 7, n / 2, n / 2 + 1, n - 1};
    const uint64_t mask[6] = {1, 0x10, 0x8000000000000000ull, 3, 0xFF00, 0x10};
    uint64_t bits = 0, stuck = 0;
    for (int k = 0; k < 6; ++k) {
      buf[at[k]] ^= mask[k];
      bits += (uint64_t)__builtin_popcountll(mask[k]);
      stuck |= mask[k];
    }
    gm_hl_host_cmp_t c;
    gm_hl_host_compare(buf.data(), n, GM_MEMTEST_RANDOM, 0, kSeed, 1, base, &c);
    EXPECT(c.words == 6 && c.bits == bits && c.stuck == stuck && c.records_filled == 6);
    for (int k = 0; k < 6 && k < (int)c.records_filled; ++k) {
      EXPECT(c.offset[k] == base + 8 * at[k]);
      EXPECT((c.expected[k] ^ c.got[k]) == mask[k]);
      EXPECT(c.got[k] == buf[at[k]]);
    }
    // more flips than records: counted, the first 16 kept in order
    for (uint64_t i = 0; i < 40; ++i) buf[100 + 1000 * i] ^= 4;
    gm_hl_host_compare(buf.data(), n, GM_MEMTEST_RANDOM, 0, kSeed, 1, base, &c);
    EXPECT(c.words == 46 && c.records_filled == 16);
    for (uint32_t k = 1; k < c.records_filled; ++k) EXPECT(c.offset[k] > c.offset[k - 1]);
    // poison overwrites every byte of its range and nothing else
    gm_hl_host_poison(buf.data() + 1, n - 2, 0xA5);
    EXPECT(buf[1] == 0xA5A5A5A5A5A5A5A5ull && buf[n - 2] == 0xA5A5A5A5A5A5A5A5ull);
    EXPECT(buf[0] != 0xA5A5A5A5A5A5A5A5ull && buf[n - 1] != 0xA5A5A5A5A5A5A5A5ull);
    bool all = true;
    for (uint64_t i = 1; i < n - 1; ++i) all &= buf[i] == 0xA5A5A5A5A5A5A5A5ull;
    EXPECT(all);
  }

  // the split covers every word exactly once, for every part count and awkward sizes
  const uint64_t counts[6] = {0, 1, 3, 4, 1001, 4 * GM_HL_HOST_WORDS_PER_THREAD + 3};
  for (uint64_t words : counts)
    for (int parts = 1; parts <= GM_HL_HOST_MAX_THREADS; ++parts) {
      uint64_t next = 0, smallest = ~0ull, largest = 0;
      for (int k = 0; k < parts; ++k) {
        uint64_t b, e;
        gm_hl_host_split(words, parts, k, &b, &e);
        EXPECT(b == next && e >= b);
        next = e;
        smallest = e - b < smallest ? e - b : smallest;
        largest = e - b > largest ? e - b : largest;
      }
      EXPECT(next == words && largest - smallest <= 1);
    }
  {
    // and the threads really write disjoint ranges: count the visits
    const uint64_t words = 1001;
    std::vector<unsigned char> hit(words, 0);
    unsigned char* h = hit.data();
    gm_hl_host_for_parts(words, 4, [h](int, uint64_t b, uint64_t e) {
      for (uint64_t i = b; i < e; ++i) ++h[i];
    });
    bool once = true;
    for (unsigned char v : hit) once &= v == 1;
    EXPECT(once);
  }

  if (failures) {
    printf("%d failure(s)\n", failures);
    return 1;
  }
  printf("test_hostlink_host: ok\n");
  return 0;
}
