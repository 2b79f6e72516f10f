// gm_atomics_ref.h — the atomics and coherence test's value functions and host reference, one
// definition for the host (gm_probe_atomics_expected, gm_probe_atomics_widths) and for the gfx950
// kernels (native/hip/gm_atomics.hip). The formulas are written out in gm_probe.h; this is their
// only implementation. The hash is the CU scan's mixer (gm_cuscan_sig.h).
#pragma once
#include <stdint.h>

#include <vector>

#include "gm_cuscan_sig.h"

#define GM_ATOMICS_HD GM_CUSCAN_HD

enum {
  GM_ATOMICS_ADD = 1,
  GM_ATOMICS_TICKET = 2,
  GM_ATOMICS_CAS = 4,
  GM_ATOMICS_HANDOFF = 8,
  GM_ATOMICS_ALL = 15,
};

// kinds: 0..9 are the ADD test's, then one per other test; COUNT is a pseudo-kind of
// gm_probe_atomics_expected (adds per word)
enum {
  GM_ATOMICS_K_ADD_U32 = 0,
  GM_ATOMICS_K_ADD_U64 = 1,
  GM_ATOMICS_K_XOR_U64 = 2,
  GM_ATOMICS_K_UMAX_U32 = 3,
  GM_ATOMICS_K_UMIN_U32 = 4,
  GM_ATOMICS_K_AND_U32 = 5,
  GM_ATOMICS_K_OR_U32 = 6,
  GM_ATOMICS_K_ADD_F32 = 7,
  GM_ATOMICS_K_ADD_F64 = 8,
  GM_ATOMICS_K_PK_ADD_BF16 = 9,
  GM_ATOMICS_ADD_KINDS = 10,
  GM_ATOMICS_K_TICKET = 10,
  GM_ATOMICS_K_CAS = 11,
  GM_ATOMICS_K_HANDOFF = 12,
  GM_ATOMICS_KINDS = 13,
  GM_ATOMICS_K_COUNT = 13,
};

#define GM_ATOMICS_THREADS 256
#define GM_ATOMICS_MAX_BLOCKS 4096
#define GM_ATOMICS_MAX_ITERS 1024          /* the hash index g * 1024 + s stays 32-bit */
#define GM_ATOMICS_DEFAULT_ITERS 8
#define GM_ATOMICS_MAX_SPREAD 65536u
#define GM_ATOMICS_DEFAULT_SPREAD 4096u
#define GM_ATOMICS_MAX_WIDTH (1u << 21)    /* a widened table */
#define GM_ATOMICS_MAX_OPS (1ull << 26)    /* T * iters: bounds the host fold and the ticket marks */
#define GM_ATOMICS_STRIDE 97u              /* a(g, s) = (g + 97 s) mod W */
#define GM_ATOMICS_FLOAT_CAP ((1ull << 22) - 1) /* 4 * adds < 2^24 */
#define GM_ATOMICS_BF16_CAP 128ull
/* CAS: with A operations into a word a thread may fail A - 1 exchanges, so the work grows with
   the square of A; the cap keeps a hot-word request in milliseconds */
#define GM_ATOMICS_CAS_CAP 1024ull
#define GM_ATOMICS_MAX_ROUNDS 64
#define GM_ATOMICS_DEFAULT_ROUNDS 8
#define GM_ATOMICS_DEFAULT_LINES 16
#define GM_ATOMICS_LINE_WORDS 1024u        /* 4 KiB: 16 bytes per thread */
#define GM_ATOMICS_FLAG_WORDS 32u          /* a flag has a 128-byte line of its own */
#define GM_ATOMICS_MAX_BUDGET_US 1000
#define GM_ATOMICS_DEFAULT_BUDGET_US 200
#define GM_ATOMICS_MAX_MAILBOX_BYTES (1ull << 30)
#define GM_ATOMICS_HASH_BASE 0x100u        /* keeps the kinds clear of the CU scan's test ids */

// H(kind, g, s); `half` 1 gives the upper 32 bits of a 64-bit operand
GM_ATOMICS_HD uint32_t gm_atomics_hash(uint64_t seed, uint32_t kind, uint32_t half, uint32_t g,
                                       uint32_t s) {
  return gm_cuscan_hash(seed, GM_ATOMICS_HASH_BASE + kind + 32u * half,
                        g * GM_ATOMICS_MAX_ITERS + s);
}

GM_ATOMICS_HD uint32_t gm_atomics_addr(uint32_t g, uint32_t s, uint32_t width) {
  return (g + GM_ATOMICS_STRIDE * s) & (width - 1u);  // width is a power of two
}

GM_ATOMICS_HD bool gm_atomics_is64(uint32_t kind) {
  return kind == GM_ATOMICS_K_ADD_U64 || kind == GM_ATOMICS_K_XOR_U64 ||
         kind == GM_ATOMICS_K_ADD_F64 || kind == GM_ATOMICS_K_CAS;
}

// what a table holds before the first operation (the byte of its memset)
GM_ATOMICS_HD uint32_t gm_atomics_init_byte(uint32_t kind) {
  return kind == GM_ATOMICS_K_UMIN_U32 || kind == GM_ATOMICS_K_AND_U32 ? 0xFFu : 0u;
}

// 64-bit integer operand: H in the low half (where a negative control's mask lands), H' above
GM_ATOMICS_HD uint64_t gm_atomics_op64(uint64_t seed, uint32_t kind, uint32_t h, uint32_t g,
                                       uint32_t s) {
  return ((uint64_t)gm_atomics_hash(seed, kind, 1, g, s) << 32) | h;
}
// or: one bit in one operation of eight; and: its complement
GM_ATOMICS_HD uint32_t gm_atomics_bit(uint32_t h) {
  return ((h >> 5) & 7u) == 0 ? 1u << (h & 31u) : 0u;
}
// float addends: an integer in [-4, 4]
GM_ATOMICS_HD int32_t gm_atomics_small(uint32_t h) { return (int32_t)(h % 9u) - 4; }
// ticket: how many tickets one draw takes
GM_ATOMICS_HD uint32_t gm_atomics_draw(uint32_t h) { return 1u + (h & 3u); }

// hand-off payload word E(b, r, word): b < 4096, r < 64, word < 16384
GM_ATOMICS_HD uint32_t gm_atomics_payload(uint64_t seed, uint32_t b, uint32_t r, uint32_t word) {
  return gm_cuscan_hash(seed, GM_ATOMICS_HASH_BASE + GM_ATOMICS_K_HANDOFF,
                        (b << 20) | (r << 14) | word);
}
// whose mailbox block b reads in round r
GM_ATOMICS_HD uint32_t gm_atomics_partner(uint32_t b, uint32_t r, uint32_t blocks) {
  return blocks == 1 ? b : (b + 1u + r % (blocks - 1u)) % blocks;
}

// ------------------------------------------------------------------------------ host only

inline bool gm_atomics_pow2(uint32_t v) { return v != 0 && (v & (v - 1)) == 0; }

inline bool gm_atomics_geometry_ok(uint32_t blocks, uint32_t iters) {
  return blocks >= 1 && blocks <= GM_ATOMICS_MAX_BLOCKS && iters >= 1 &&
         iters <= GM_ATOMICS_MAX_ITERS &&
         (uint64_t)blocks * GM_ATOMICS_THREADS * iters <= GM_ATOMICS_MAX_OPS;
}

// operations per word of a table of `width` words: count[w] = |{(g, s): a(g, s) = w}|
inline void gm_atomics_counts(uint32_t blocks, uint32_t iters, uint32_t width,
                              std::vector<uint32_t>& count) {
  const uint32_t T = blocks * GM_ATOMICS_THREADS;
  std::vector<int64_t> diff((size_t)width + 1, 0);
  const uint32_t laps = T / width, rem = T % width;
  for (uint32_t s = 0; s < iters; ++s) {
    const uint32_t first = (GM_ATOMICS_STRIDE * s) & (width - 1u);
    if (rem == 0) continue;
    if (first + rem <= width) {
      ++diff[first], --diff[first + rem];
    } else {
      ++diff[first], --diff[width];
      ++diff[0], --diff[first + rem - width];
    }
  }
  count.assign(width, 0);
  int64_t run = 0;
  for (uint32_t w = 0; w < width; ++w) {
    run += diff[w];
    count[w] = (uint32_t)(run + (int64_t)laps * iters);
  }
}

inline uint64_t gm_atomics_max_adds(uint32_t blocks, uint32_t iters, uint32_t width) {
  std::vector<uint32_t> c;
  gm_atomics_counts(blocks, iters, width, c);
  uint64_t m = 0;
  for (uint32_t v : c) m = v > m ? v : m;
  return m;
}

// adds into one word that keep the kind exact in any order (CAS: that keep its retries few);
// 0: no cap
inline uint64_t gm_atomics_cap(uint32_t kind) {
  if (kind == GM_ATOMICS_K_CAS) return GM_ATOMICS_CAS_CAP;
  if (kind == GM_ATOMICS_K_ADD_F32 || kind == GM_ATOMICS_K_ADD_F64) return GM_ATOMICS_FLOAT_CAP;
  if (kind == GM_ATOMICS_K_PK_ADD_BF16) return GM_ATOMICS_BF16_CAP;
  return 0;
}

// the table width of `kind` for a requested spread: the smallest power of two >= spread whose
// busiest word stays within the kind's cap; 0 when none up to GM_ATOMICS_MAX_WIDTH does
inline uint32_t gm_atomics_width(uint32_t kind, uint32_t blocks, uint32_t iters, uint32_t spread) {
  const uint64_t cap = gm_atomics_cap(kind);
  if (cap == 0) return spread;
  for (uint32_t w = spread; w != 0 && w <= GM_ATOMICS_MAX_WIDTH; w <<= 1)
    if (gm_atomics_max_adds(blocks, iters, w) <= cap) return w;
  return 0;
}

inline bool gm_atomics_width_ok(uint32_t kind, uint32_t blocks, uint32_t iters, uint32_t width) {
  if (!gm_atomics_pow2(width) || width > GM_ATOMICS_MAX_WIDTH) return false;
  const uint64_t cap = gm_atomics_cap(kind);
  return cap == 0 || gm_atomics_max_adds(blocks, iters, width) <= cap;
}

inline uint32_t gm_atomics_f32_bits(float f) { return gm_cuscan_f32_bits(f); }
inline uint64_t gm_atomics_f64_bits(double d) {
  uint64_t u;
  __builtin_memcpy(&u, &d, 8);
  return u;
}

// The final table of `kind` (any GM_ATOMICS_K_* but HANDOFF), folded in (s, g) order; the
// operations commute, so any order gives the same words. `out` holds `width` words of 4 or 8 bytes
// (gm_atomics_is64). TICKET: the counters' final values N_k. COUNT: the operations per word.
// A negative control (inj_mask != 0) XORs H of operation (inj_g, inj_s). The caller has checked
// the geometry and the width.
inline void gm_atomics_expected_host(uint32_t kind, uint32_t blocks, uint32_t iters,
                                     uint32_t width, uint64_t seed, uint32_t inj_g, uint32_t inj_s,
                                     uint32_t inj_mask, void* out) {
  const uint32_t T = blocks * GM_ATOMICS_THREADS;
  uint32_t* o32 = (uint32_t*)out;
  uint64_t* o64 = (uint64_t*)out;
  if (kind == GM_ATOMICS_K_COUNT) {
    std::vector<uint32_t> c;
    gm_atomics_counts(blocks, iters, width, c);
    for (uint32_t w = 0; w < width; ++w) o32[w] = c[w];
    return;
  }
  std::vector<int64_t> sum;   // the float kinds add integers
  std::vector<uint32_t> half; // the bf16 halves count ones
  if (kind == GM_ATOMICS_K_ADD_F32 || kind == GM_ATOMICS_K_ADD_F64) sum.assign(width, 0);
  if (kind == GM_ATOMICS_K_PK_ADD_BF16) half.assign(2 * (size_t)width, 0);
  const uint32_t init32 = gm_atomics_init_byte(kind) ? 0xFFFFFFFFu : 0u;
  for (uint32_t w = 0; w < width; ++w) {
    if (gm_atomics_is64(kind)) o64[w] = 0; else o32[w] = init32;
  }
  for (uint32_t s = 0; s < iters; ++s)
    for (uint32_t g = 0; g < T; ++g) {
      uint32_t h = gm_atomics_hash(seed, kind, 0, g, s);
      if (inj_mask != 0 && g == inj_g && s == inj_s) h ^= inj_mask;
      const uint32_t w = gm_atomics_addr(g, s, width);
      switch (kind) {
        case GM_ATOMICS_K_ADD_U32: o32[w] += h; break;
        case GM_ATOMICS_K_ADD_U64:
        case GM_ATOMICS_K_CAS: o64[w] += gm_atomics_op64(seed, kind, h, g, s); break;
        case GM_ATOMICS_K_XOR_U64: o64[w] ^= gm_atomics_op64(seed, kind, h, g, s); break;
        case GM_ATOMICS_K_UMAX_U32: o32[w] = h > o32[w] ? h : o32[w]; break;
        case GM_ATOMICS_K_UMIN_U32: o32[w] = h < o32[w] ? h : o32[w]; break;
        case GM_ATOMICS_K_AND_U32: o32[w] &= ~gm_atomics_bit(h); break;
        case GM_ATOMICS_K_OR_U32: o32[w] |= gm_atomics_bit(h); break;
        case GM_ATOMICS_K_ADD_F32:
        case GM_ATOMICS_K_ADD_F64: sum[w] += gm_atomics_small(h); break;
        case GM_ATOMICS_K_PK_ADD_BF16:
          half[2 * (size_t)w] += h & 1u;
          half[2 * (size_t)w + 1] += (h >> 1) & 1u;
          break;
        case GM_ATOMICS_K_TICKET: o32[w] += gm_atomics_draw(h); break;
        default: break;
      }
    }
  for (uint32_t w = 0; w < width; ++w) {
    if (kind == GM_ATOMICS_K_ADD_F32) o32[w] = gm_atomics_f32_bits((float)sum[w]);
    if (kind == GM_ATOMICS_K_ADD_F64) o64[w] = gm_atomics_f64_bits((double)sum[w]);
    if (kind == GM_ATOMICS_K_PK_ADD_BF16)  // an integer <= 256 has at most 8 significant bits
      o32[w] = (gm_atomics_f32_bits((float)half[2 * (size_t)w]) >> 16) |
               (gm_atomics_f32_bits((float)half[2 * (size_t)w + 1]) & 0xFFFF0000u);
  }
}
