// gm_hostlink_host.h — host side of the host-link test (native/hip/gm_hostlink.hip): fill a host
// buffer with a memtest pattern and compare one against it. Plain C++, no HIP, so that it can be
// tested alone (native/tests/test_hostlink_host.cpp). Every expected value comes from
// gm_memtest_expected (gm_memtest_pattern.h).
//
// Large buffers are split over a few std::threads: contiguous word ranges, at most
// GM_HL_HOST_MAX_THREADS of them, one more per GM_HL_HOST_WORDS_PER_THREAD words. The count is a
// function of the size alone, never of the machine.
#pragma once
#include <stdint.h>
#include <string.h>

#include <thread>

#include "gm_memtest_pattern.h"

#define GM_HL_HOST_MAX_THREADS 4
#define GM_HL_HOST_WORDS_PER_THREAD (1ull << 20)  // 8 MiB
#define GM_HL_HOST_MAX_RECORDS 16

// What a compare found. Records are in ascending offset order.
typedef struct gm_hl_host_cmp {
  uint64_t words;  // 64-bit words that differed
  uint64_t bits;   // sum of popcount(expected ^ got)
  uint64_t stuck;  // OR of expected ^ got
  uint32_t records_filled;
  uint64_t offset[GM_HL_HOST_MAX_RECORDS];  // global byte offset
  uint64_t expected[GM_HL_HOST_MAX_RECORDS];
  uint64_t got[GM_HL_HOST_MAX_RECORDS];
} gm_hl_host_cmp_t;

inline int gm_hl_host_threads(uint64_t n_words) {
  const uint64_t t = n_words / GM_HL_HOST_WORDS_PER_THREAD;
  return t < 1 ? 1 : t > GM_HL_HOST_MAX_THREADS ? GM_HL_HOST_MAX_THREADS : (int)t;
}

// Part k of `parts`: words [*begin, *end). The parts are contiguous, disjoint and cover
// [0, n_words); their sizes differ by at most one word.
inline void gm_hl_host_split(uint64_t n_words, int parts, int k, uint64_t* begin, uint64_t* end) {
  const uint64_t q = n_words / (uint64_t)parts, r = n_words % (uint64_t)parts;
  const uint64_t uk = (uint64_t)k;
  *begin = uk * q + (uk < r ? uk : r);
  *end = *begin + q + (uk < r ? 1 : 0);
}

// Runs fn(k, begin, end) for every part, part 0 on the calling thread.
template <class Fn>
inline void gm_hl_host_for_parts(uint64_t n_words, int parts, Fn fn) {
  std::thread th[GM_HL_HOST_MAX_THREADS];
  for (int k = 1; k < parts; ++k) {
    uint64_t b, e;
    gm_hl_host_split(n_words, parts, k, &b, &e);
    th[k] = std::thread(fn, k, b, e);
  }
  uint64_t b, e;
  gm_hl_host_split(n_words, parts, 0, &b, &e);
  fn(0, b, e);
  for (int k = 1; k < parts; ++k) th[k].join();
}

inline void gm_hl_host_fill_range(uint64_t* buf, uint64_t begin, uint64_t end, uint32_t pattern,
                                  uint64_t inv, uint64_t seed, uint32_t pass, uint64_t base) {
  for (uint64_t i = begin; i < end; ++i)
    buf[i] = gm_memtest_expected(pattern, seed, pass, base + 8 * i) ^ inv;
}

// buf[i] = P(base_offset + 8 i), or ~P with `invert`.
inline void gm_hl_host_fill(uint64_t* buf, uint64_t n_words, uint32_t pattern, int invert,
                            uint64_t seed, uint32_t pass, uint64_t base_offset) {
  const uint64_t inv = invert ? ~0ull : 0ull;
  gm_hl_host_for_parts(n_words, gm_hl_host_threads(n_words),
                       [=](int, uint64_t b, uint64_t e) {
                         gm_hl_host_fill_range(buf, b, e, pattern, inv, seed, pass, base_offset);
                       });
}

// Every byte of the buffer = `byte`: what a destination holds before a transfer must overwrite it.
inline void gm_hl_host_poison(uint64_t* buf, uint64_t n_words, int byte) {
  gm_hl_host_for_parts(n_words, gm_hl_host_threads(n_words), [=](int, uint64_t b, uint64_t e) {
    memset(buf + b, byte, (size_t)(e - b) * 8);
  });
}

inline void gm_hl_host_compare_range(const uint64_t* buf, uint64_t begin, uint64_t end,
                                     uint32_t pattern, uint64_t inv, uint64_t seed, uint32_t pass,
                                     uint64_t base, gm_hl_host_cmp_t* out) {
  for (uint64_t i = begin; i < end; ++i) {
    const uint64_t o = base + 8 * i;
    const uint64_t e = gm_memtest_expected(pattern, seed, pass, o) ^ inv, g = buf[i];
    if (e == g) continue;
    const uint64_t x = e ^ g;
    ++out->words;
    out->bits += (uint64_t)__builtin_popcountll(x);
    out->stuck |= x;
    if (out->records_filled < GM_HL_HOST_MAX_RECORDS) {
      const uint32_t s = out->records_filled++;
      out->offset[s] = o;
      out->expected[s] = e;
      out->got[s] = g;
    }
  }
}

// Adds `part` (found in words after those of *into) to *into.
inline void gm_hl_host_merge(gm_hl_host_cmp_t* into, const gm_hl_host_cmp_t* part) {
  into->words += part->words;
  into->bits += part->bits;
  into->stuck |= part->stuck;
  for (uint32_t i = 0;
       i < part->records_filled && into->records_filled < GM_HL_HOST_MAX_RECORDS; ++i) {
    const uint32_t s = into->records_filled++;
    into->offset[s] = part->offset[i];
    into->expected[s] = part->expected[i];
    into->got[s] = part->got[i];
  }
}

// Compares buf against P (or ~P); *out is overwritten.
inline void gm_hl_host_compare(const uint64_t* buf, uint64_t n_words, uint32_t pattern, int invert,
                               uint64_t seed, uint32_t pass, uint64_t base_offset,
                               gm_hl_host_cmp_t* out) {
  const uint64_t inv = invert ? ~0ull : 0ull;
  gm_hl_host_cmp_t part[GM_HL_HOST_MAX_THREADS];
  memset(part, 0, sizeof(part));
  const int parts = gm_hl_host_threads(n_words);
  gm_hl_host_for_parts(n_words, parts, [=, &part](int k, uint64_t b, uint64_t e) {
    gm_hl_host_compare_range(buf, b, e, pattern, inv, seed, pass, base_offset, &part[k]);
  });
  memset(out, 0, sizeof(*out));
  for (int k = 0; k < parts; ++k) gm_hl_host_merge(out, &part[k]);
}
