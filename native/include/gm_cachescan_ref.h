// gm_cachescan_ref.h — the cache scan's value model: test bits, geometry, the data formulas (one
// definition for the host and for the gfx950 kernel, native/hip/gm_cachescan.hip) and the host
// evaluation of a block's expected table, with or without a poked word.
// The formulas are written out in gm_probe.h; this is their only implementation.
//
// What is shared is data: hashes, address permutations, the folds, the instruction-cache body's
// literals. What is under test is not here at all: on the device a value passes through the
// vector L1, the L2, the scalar data cache or the instruction cache; the host keeps the segment
// and the table in plain arrays and never reads what the device wrote.
#pragma once
#include <stdint.h>

#include "gm_cuscan_sig.h"

enum {
  GM_CACHESCAN_L2 = 1,      // march over the segment, every load served by the L2
  GM_CACHESCAN_L1 = 2,      // hit passes and a replacement sweep through the vector L1
  GM_CACHESCAN_SCALAR = 4,  // a pointer chase through the scalar data cache
  GM_CACHESCAN_ICACHE = 8,  // a straight-line body larger than the instruction cache
  GM_CACHESCAN_ALL = 15,
};
enum { GM_CACHESCAN_IX_L2, GM_CACHESCAN_IX_L1, GM_CACHESCAN_IX_SCALAR, GM_CACHESCAN_IX_ICACHE };

#define GM_CACHESCAN_TESTS 4
/* measured on an MI355X (profiles/cachescan/README.md): a round of all four tests takes
   0.53 ms at 4, 0.20 ms at 1 and 6.67 ms at 63; the other scans' default rounds take 0.1-0.6 ms */
#define GM_CACHESCAN_DEFAULT_ITERS 4
#define GM_CACHESCAN_MAX_ITERS 63
/* hash test ids: disjoint from the CU scan's (1..8), the atomics' (0x100..), the format scan's
   (0x200..) and the lane scan's (0x300..) */
#define GM_CACHESCAN_H_PATTERN 0x400u
#define GM_CACHESCAN_H_KEY 0x401u
#define GM_CACHESCAN_H_TABLE 0x410u
#define GM_CACHESCAN_H_SCALAR 0x411u
#define GM_CACHESCAN_H_SCALAR_LANE 0x412u
#define GM_CACHESCAN_H_ICACHE 0x420u

// One segment of the arena per block; the pattern index 65536 r + a holds a word address.
#define GM_CACHESCAN_SEG_BYTES 65536
#define GM_CACHESCAN_SEG_WORDS (GM_CACHESCAN_SEG_BYTES / 4)
#define GM_CACHESCAN_SEG_VECS (GM_CACHESCAN_SEG_BYTES / 16)
#define GM_CACHESCAN_L2_STRIDE 6151u        /* odd: coprime to 16384 */
#define GM_CACHESCAN_L2_OFFSET 3u
#define GM_CACHESCAN_L1_HIT_BYTES 16384     /* half of the 32 KiB the L1 is taken to hold */
#define GM_CACHESCAN_L1_HIT_WORDS (GM_CACHESCAN_L1_HIT_BYTES / 4)
#define GM_CACHESCAN_L1_ROUND 64u           /* l1's pattern round: beyond l2's 0..62 */
#define GM_CACHESCAN_L1_HIT_STRIDE 389u     /* odd: coprime to 1024 */
#define GM_CACHESCAN_L1_HIT_OFFSET 11u
#define GM_CACHESCAN_L1_SWEEP_STRIDE 4099u  /* odd: coprime to 16384 */
#define GM_CACHESCAN_L1_SWEEP_OFFSET 5u
#define GM_CACHESCAN_TABLE_BYTES 32768      /* the scalar test's table: larger than its cache */
#define GM_CACHESCAN_TABLE_WORDS (GM_CACHESCAN_TABLE_BYTES / 4)
#define GM_CACHESCAN_SCALAR_STEPS 64        /* per unit of iters */
#define GM_CACHESCAN_ICACHE_STEPS 3072      /* distinct steps of the straight-line body */

static_assert(GM_CACHESCAN_MAX_ITERS <= GM_CACHESCAN_L1_ROUND, "l1's round is not one of l2's");
static_assert(GM_CACHESCAN_SEG_WORDS <= 65536, "a word address fits the pattern index");
static_assert(GM_CACHESCAN_SEG_VECS % GM_CUSCAN_THREADS == 0 &&
                  GM_CACHESCAN_L1_HIT_WORDS % (4 * GM_CUSCAN_THREADS) == 0,
              "whole steps per thread");

GM_CUSCAN_HD uint32_t gm_cachescan_fold(uint32_t s, uint32_t v) {
  return gm_cuscan_rotl32(s, 5) + v;
}

// ================================================================================ the arena
// Word a of segment b holds pattern(r, a) ^ key(b); the kernel removes the key before it folds.
GM_CUSCAN_HD uint32_t gm_cachescan_pattern(uint64_t seed, uint32_t round, uint32_t addr) {
  return gm_cuscan_hash(seed, GM_CACHESCAN_H_PATTERN, round * 65536u + addr);
}
GM_CUSCAN_HD uint32_t gm_cachescan_key(uint64_t seed, uint32_t block) {
  return gm_cuscan_hash(seed, GM_CACHESCAN_H_KEY, block);
}
// 16-byte element thread t fills in step k
GM_CUSCAN_HD uint32_t gm_cachescan_fill_vec(uint32_t t, uint32_t k) { return k * 256u + t; }

// ================================================================================ l2
// word read and inverted by thread t in step i of phase 2: each word once
GM_CUSCAN_HD uint32_t gm_cachescan_l2_perm(uint32_t j) {
  return (j * GM_CACHESCAN_L2_STRIDE + GM_CACHESCAN_L2_OFFSET) % GM_CACHESCAN_SEG_WORDS;
}
// 16-byte element read back in step k of phase 3: filled by the next wave
GM_CUSCAN_HD uint32_t gm_cachescan_l2_vec(uint32_t t, uint32_t k) {
  return k * 256u + ((t + 64u) & 255u);
}
// the folds are the CU scan's LDS march's: gm_cuscan_lds_fold32, gm_cuscan_lds_fold128

// ================================================================================ l1
// Wave w filled the words a with (a / 256) % 4 == w. In the hit phase thread t of wave w reads,
// in step i, a word the next wave filled; the 1024 (step, lane) pairs of a wave are a permutation
// of that wave's 1024 words of the first 16 KiB.
GM_CUSCAN_HD uint32_t gm_cachescan_l1_hit_addr(uint32_t t, uint32_t i) {
  const uint32_t w = t >> 6, l = t & 63u;
  const uint32_t j = ((64u * i + l) * GM_CACHESCAN_L1_HIT_STRIDE + GM_CACHESCAN_L1_HIT_OFFSET) & 1023u;
  return 1024u * (j >> 8) + 256u * ((w + 1u) & 3u) + (j & 255u);
}
// word read twice by thread t in step i of the replacement sweep: each word of the segment once
GM_CUSCAN_HD uint32_t gm_cachescan_l1_sweep_addr(uint32_t t, uint32_t i) {
  return ((256u * i + t) * GM_CACHESCAN_L1_SWEEP_STRIDE + GM_CACHESCAN_L1_SWEEP_OFFSET) %
         GM_CACHESCAN_SEG_WORDS;
}
// one probe: `l1` came through the L1, `l2` is the same word by the bypass load
GM_CUSCAN_HD void gm_cachescan_l1_fold(uint32_t s[4], uint32_t l1, uint32_t l2, uint32_t want) {
  s[0] = gm_cachescan_fold(s[0], l1);
  s[1] = gm_cachescan_fold(s[1], l2);
  s[2] += l1 != l2;
  s[3] += l1 != want;
}

// ================================================================================ scalar
GM_CUSCAN_HD uint32_t gm_cachescan_table(uint64_t seed, uint32_t i) {
  return gm_cuscan_hash(seed, GM_CACHESCAN_H_TABLE, i);
}
struct gm_cachescan_chain {
  uint32_t i, a, b;
};
GM_CUSCAN_HD gm_cachescan_chain gm_cachescan_scalar_init(uint64_t seed, uint32_t w) {
  gm_cachescan_chain c;
  c.i = gm_cuscan_hash(seed, GM_CACHESCAN_H_SCALAR, 4 * w) % GM_CACHESCAN_TABLE_WORDS;
  c.a = gm_cuscan_hash(seed, GM_CACHESCAN_H_SCALAR, 4 * w + 1);
  c.b = gm_cuscan_hash(seed, GM_CACHESCAN_H_SCALAR, 4 * w + 2);
  return c;
}
// step s with k = T[c.i], the word just read: the next index depends on it
GM_CUSCAN_HD void gm_cachescan_scalar_step(gm_cachescan_chain& c, uint32_t s, uint32_t k) {
  c.a = gm_cuscan_rotl32(c.a, 5) + k;
  c.b = (c.b ^ c.a) * 0x9E3779B1u;
  c.b ^= c.b >> 15;
  uint32_t m = ((c.i ^ k) + s) * 0x85EBCA6Bu;
  m ^= m >> 13;
  c.i = m % GM_CACHESCAN_TABLE_WORDS;
}
GM_CUSCAN_HD void gm_cachescan_scalar_fold(uint32_t v[4], uint32_t s, uint32_t l,
                                           const gm_cachescan_chain& c) {
  v[s & 3] = gm_cuscan_rotl32(v[s & 3], 7) + (c.a ^ l * 0x01000193u);
  v[(s + 2) & 3] ^= c.b + l;
}

// ================================================================================ icache
// Literal n (0..2) of step j. In the kernel j is a template argument and these are immediates.
constexpr uint32_t gm_cachescan_ic_const(uint32_t j, uint32_t n) {
  uint32_t h = (4u * j + n) * 0x9E3779B1u + 0x7F4A7C15u;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
GM_CUSCAN_HD void gm_cachescan_ic_step(uint32_t j, uint32_t& x, uint32_t& y) {
  x = gm_cuscan_rotl32(x, 1 + (int)(j % 31u)) + gm_cachescan_ic_const(j, 0);
  x ^= y;
  x *= gm_cachescan_ic_const(j, 1) | 1u;
  y = gm_cuscan_rotl32(y, 1 + (int)((j / 31u) % 31u)) ^ x;
  y += gm_cachescan_ic_const(j, 2);
}

// ---- host evaluation of a whole block's table, out[4 t + i]; `test` one GM_CACHESCAN_* bit and
// iters within its bound (the entry points check both). poke_mask != 0: the run in which
// poke_mask was XORed into word poke_offset of the segment after the test's (first) fill, or of
// the scalar test's table; the offset is inside the segment or table.
inline void gm_cachescan_expected_host(uint32_t test, uint64_t seed, uint32_t iters,
                                       uint32_t poke_offset, uint32_t poke_mask,
                                       uint32_t out[GM_CUSCAN_SIG_WORDS]) {
  const uint32_t T = GM_CUSCAN_THREADS;
  for (uint32_t i = 0; i < GM_CUSCAN_SIG_WORDS; ++i) out[i] = 0;
  if (test == GM_CACHESCAN_L2) {
    static thread_local uint32_t seg[GM_CACHESCAN_SEG_WORDS];
    for (uint32_t r = 0; r < iters; ++r) {
      for (uint32_t a = 0; a < GM_CACHESCAN_SEG_WORDS; ++a) seg[a] = gm_cachescan_pattern(seed, r, a);
      if (r == 0) seg[poke_offset] ^= poke_mask;
      for (uint32_t t = 0; t < T; ++t)
        for (uint32_t i = 0; i < GM_CACHESCAN_SEG_WORDS / T; ++i) {
          const uint32_t a = gm_cachescan_l2_perm(i * 256 + t);
          const uint32_t g = seg[a];
          gm_cuscan_lds_fold32(out + 4 * t, g, gm_cachescan_pattern(seed, r, a));
          seg[a] = ~g;
        }
      for (uint32_t t = 0; t < T; ++t)
        for (uint32_t k = 0; k < GM_CACHESCAN_SEG_VECS / T; ++k)
          for (uint32_t c = 0; c < 4; ++c) {
            const uint32_t a = 4 * gm_cachescan_l2_vec(t, k) + c;
            gm_cuscan_lds_fold128(out + 4 * t, seg[a], ~gm_cachescan_pattern(seed, r, a));
          }
    }
  } else if (test == GM_CACHESCAN_L1) {
    static thread_local uint32_t seg[GM_CACHESCAN_SEG_WORDS];
    for (uint32_t a = 0; a < GM_CACHESCAN_SEG_WORDS; ++a)
      seg[a] = gm_cachescan_pattern(seed, GM_CACHESCAN_L1_ROUND, a);
    seg[poke_offset] ^= poke_mask;
    for (uint32_t t = 0; t < T; ++t) {
      uint32_t* s = out + 4 * t;
      for (uint32_t pass = 0; pass < iters; ++pass)
        for (uint32_t i = 0; i < GM_CACHESCAN_L1_HIT_WORDS / T; ++i) {
          const uint32_t a = gm_cachescan_l1_hit_addr(t, i);
          gm_cachescan_l1_fold(s, seg[a], seg[a], gm_cachescan_pattern(seed, GM_CACHESCAN_L1_ROUND, a));
        }
      for (uint32_t i = 0; i < GM_CACHESCAN_SEG_WORDS / T; ++i) {
        const uint32_t a = gm_cachescan_l1_sweep_addr(t, i);
        const uint32_t want = gm_cachescan_pattern(seed, GM_CACHESCAN_L1_ROUND, a);
        gm_cachescan_l1_fold(s, seg[a], seg[a], want);
        gm_cachescan_l1_fold(s, seg[a], seg[a], want);
      }
    }
  } else if (test == GM_CACHESCAN_SCALAR) {
    static thread_local uint32_t table[GM_CACHESCAN_TABLE_WORDS];
    for (uint32_t i = 0; i < GM_CACHESCAN_TABLE_WORDS; ++i) table[i] = gm_cachescan_table(seed, i);
    table[poke_offset] ^= poke_mask;
    for (uint32_t t = 0; t < T; ++t)
      for (uint32_t i = 0; i < 4; ++i)
        out[4 * t + i] = gm_cuscan_hash(seed, GM_CACHESCAN_H_SCALAR_LANE, 4 * t + i);
    for (uint32_t w = 0; w < T / 64; ++w) {
      gm_cachescan_chain c = gm_cachescan_scalar_init(seed, w);
      for (uint32_t s = 0; s < iters * GM_CACHESCAN_SCALAR_STEPS; ++s) {
        gm_cachescan_scalar_step(c, s, table[c.i]);
        for (uint32_t l = 0; l < 64; ++l) gm_cachescan_scalar_fold(out + 4 * (64 * w + l), s, l, c);
      }
    }
  } else if (test == GM_CACHESCAN_ICACHE) {
    for (uint32_t t = 0; t < T; ++t) {
      uint32_t x = gm_cuscan_hash(seed, GM_CACHESCAN_H_ICACHE, 2 * t);
      uint32_t y = gm_cuscan_hash(seed, GM_CACHESCAN_H_ICACHE, 2 * t + 1);
      uint32_t sx = 0, sy = 0;
      for (uint32_t it = 0; it < iters; ++it) {
        for (uint32_t j = 0; j < GM_CACHESCAN_ICACHE_STEPS; ++j) gm_cachescan_ic_step(j, x, y);
        sx = gm_cachescan_fold(sx, x);
        sy = gm_cachescan_fold(sy, y);
      }
      out[4 * t] = x;
      out[4 * t + 1] = y;
      out[4 * t + 2] = sx;
      out[4 * t + 3] = sy;
    }
  }
}
