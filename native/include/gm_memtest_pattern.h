// gm_memtest_pattern.h — the HBM pattern test's expected-value function, one definition for the
// host (gm_probe_memtest_expected) and for the gfx950 kernels (native/hip/gm_memtest.hip).
// The formulas are written out in gm_probe.h; this is their only implementation.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GM_MEMTEST_HD __host__ __device__ inline
#else
#define GM_MEMTEST_HD inline
#endif

enum {
  GM_MEMTEST_ADDR = 1,
  GM_MEMTEST_SOLID = 2,
  GM_MEMTEST_CHECKER = 4,
  GM_MEMTEST_WALK = 8,
  GM_MEMTEST_RANDOM = 16,
  GM_MEMTEST_ALL = 31,
};

GM_MEMTEST_HD uint32_t gm_memtest_rotl32(uint32_t v, int s) { return (v << s) | (v >> (32 - s)); }

// `random`: four add-rotate-xor rounds over the two 32-bit halves of the word index. No multiply
// (32-bit integer multiplies are not full rate on CDNA4 and a 64-bit one is several of them), no
// state, no table; each round is invertible, so for a fixed (seed, pass) two different word
// indices never get the same value.
GM_MEMTEST_HD uint64_t gm_memtest_mix(uint64_t w, uint64_t seed, uint32_t pass) {
  const uint64_t v = w ^ seed ^ ((uint64_t)(pass * 0x9E3779B9u) << 32);
  uint32_t x = (uint32_t)v, y = (uint32_t)(v >> 32);
  const uint32_t c[4] = {0x9E3779B9u, 0x85EBCA6Bu, 0xC2B2AE35u, 0x27D4EB2Fu};
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
  for (int r = 0; r < 4; ++r) {
    x = (gm_memtest_rotl32(x, 24) + y) ^ c[r];
    y = gm_memtest_rotl32(y, 3) ^ x;
  }
  return ((uint64_t)y << 32) | x;
}

// Value of the 64-bit word at global byte offset `o` (a multiple of 8) of the test region.
// `pattern` is one GM_MEMTEST_* bit; anything else gives 0 (the entry points reject it earlier).
GM_MEMTEST_HD uint64_t gm_memtest_expected(uint32_t pattern, uint64_t seed, uint32_t pass,
                                           uint64_t o) {
  const uint64_t w = o >> 3;
  switch (pattern) {
    case GM_MEMTEST_ADDR: return o ^ seed;
    case GM_MEMTEST_SOLID: return 0;
    case GM_MEMTEST_CHECKER: return 0x5555555555555555ull;
    case GM_MEMTEST_WALK: return 1ull << ((w + pass) & 63);
    case GM_MEMTEST_RANDOM: return gm_memtest_mix(w, seed, pass);
    default: return 0;
  }
}
