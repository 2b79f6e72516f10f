// gm_mfmascan_ref.h — the matrix-core format scan's value model: format bits, caps, code tables,
// the operand register images (one definition for the host and for the gfx950 kernel,
// native/hip/gm_mfmascan.hip) and the host evaluation of a block's expected table.
// The formulas are written out in gm_probe.h; this is their only implementation.
//
// Every operand is chosen so that each product and each partial sum is exactly representable in
// the accumulator type: the result is one definite bit pattern in any summation order.
#pragma once
#include <stdint.h>

#include "gm_cuscan_sig.h"

enum {
  GM_MFMASCAN_F16 = 1,      // v_mfma_f32_16x16x32_f16
  GM_MFMASCAN_FP8 = 2,      // v_mfma_f32_16x16x32_fp8_fp8 (OCP e4m3)
  GM_MFMASCAN_BF8 = 4,      // v_mfma_f32_16x16x32_bf8_bf8 (e5m2)
  GM_MFMASCAN_I8 = 8,       // v_mfma_i32_16x16x64_i8
  GM_MFMASCAN_F32 = 16,     // v_mfma_f32_16x16x4_f32
  GM_MFMASCAN_F64 = 32,     // v_mfma_f64_16x16x4_f64
  GM_MFMASCAN_MXFP8 = 64,   // v_mfma_scale_f32_16x16x128_f8f6f4, cbsz = blgp = 0 (e4m3)
  GM_MFMASCAN_MXBF8 = 128,  // the same, 1 (e5m2)
  GM_MFMASCAN_MXFP6 = 256,  // the same, 2 (e2m3)
  GM_MFMASCAN_MXBF6 = 512,  // the same, 3 (e3m2)
  GM_MFMASCAN_MXFP4 = 1024, // the same, 4 (e2m1)
  GM_MFMASCAN_ALL = 2047,
};

#define GM_MFMASCAN_FORMATS 11
#define GM_MFMASCAN_DEFAULT_ITERS 16
#define GM_MFMASCAN_MAX_ITERS 63       /* the smallest of the caps below (f32) */
#define GM_MFMASCAN_TEST_BASE 0x200u   /* hash test ids: disjoint from the CU scan's (1..8) and */
#define GM_MFMASCAN_SCALE_BASE 0x220u  /* the atomics' (0x100..0x13f) */

// Format indices: bit = 1 << index.
enum {
  GM_MFMASCAN_IX_F16, GM_MFMASCAN_IX_FP8, GM_MFMASCAN_IX_BF8, GM_MFMASCAN_IX_I8,
  GM_MFMASCAN_IX_F32, GM_MFMASCAN_IX_F64, GM_MFMASCAN_IX_MXFP8, GM_MFMASCAN_IX_MXBF8,
  GM_MFMASCAN_IX_MXFP6, GM_MFMASCAN_IX_MXBF6, GM_MFMASCAN_IX_MXFP4,
};

// Element encodings of the nibble formats.
enum {
  GM_MFMASCAN_ENC_F16, GM_MFMASCAN_ENC_E4M3, GM_MFMASCAN_ENC_E5M2, GM_MFMASCAN_ENC_E2M3,
  GM_MFMASCAN_ENC_E3M2, GM_MFMASCAN_ENC_E2M1, GM_MFMASCAN_ENCODINGS,
};

// ---- caps. A nibble element is an e2m1 value, at most 6 in magnitude, that is 12 half units: a
// product is at most 12 * 12 = 144 quarter units. An output sums K products per step.
#define GM_MFMASCAN_NIBBLE_MAX_PRODUCT 144   /* quarter units */
#define GM_MFMASCAN_F32_MAX 255              /* |integer operand| */
#define GM_MFMASCAN_F64_MAX (1 << 22)
static_assert(144ull * 128 * GM_MFMASCAN_MAX_ITERS < (1ull << 24),
              "nibble formats: every partial sum is an exact fp32 (K = 128 is the widest)");
static_assert(144ull * 128 * 910 < (1ull << 24) && 144ull * 128 * 911 >= (1ull << 24),
              "nibble formats: the cap at K = 128 is 910 steps");
static_assert(128ull * 128 * 64 * GM_MFMASCAN_MAX_ITERS < (1ull << 31),
              "i8: |product| <= 2^14, 64 per step: the sum stays inside an int32");
static_assert(4ull * GM_MFMASCAN_F32_MAX * GM_MFMASCAN_F32_MAX * GM_MFMASCAN_MAX_ITERS <
                  (1ull << 24),
              "f32: every partial sum is an exact fp32 integer");
static_assert(4ull * GM_MFMASCAN_F32_MAX * GM_MFMASCAN_F32_MAX * (GM_MFMASCAN_MAX_ITERS + 2) >=
                  (1ull << 24),
              "f32 is the format that sets GM_MFMASCAN_MAX_ITERS");
static_assert(4ull * GM_MFMASCAN_F64_MAX * GM_MFMASCAN_F64_MAX * GM_MFMASCAN_MAX_ITERS <
                  (1ull << 53),
              "f64: every partial sum is an exact fp64 integer");

// ---- code tables. Nibble n stands for the e2m1 value of n: magnitude {0, 1/2, 1, 3/2, 2, 3, 4, 6}
// [n & 7], negative when bit 3 is set (so -0 occurs). Each encoding holds all 16 exactly; byte
// n & 7 of the constant is the magnitude's code, the sign is one more bit. An f16 code is the
// e5m2 code in the upper byte of the half word (e5m2 is a truncated f16).
GM_CUSCAN_HD uint32_t gm_mfmascan_code(int enc, uint32_t n) {
  const uint64_t mag = enc == GM_MFMASCAN_ENC_E4M3   ? 0x4C4844403C383000ull
                       : enc == GM_MFMASCAN_ENC_E2M3 ? 0x1C1814100C080400ull
                       : enc == GM_MFMASCAN_ENC_E3M2 ? 0x161412100E0C0800ull
                       : enc == GM_MFMASCAN_ENC_E2M1 ? 0x0706050403020100ull
                                                     : 0x464442403E3C3800ull;  // e5m2, f16
  const uint32_t m = (uint32_t)(mag >> (8 * (n & 7u))) & 0xFFu, s = (n >> 3) & 1u;
  switch (enc) {
    case GM_MFMASCAN_ENC_F16: return m << 8 | s << 15;
    case GM_MFMASCAN_ENC_E4M3:
    case GM_MFMASCAN_ENC_E5M2: return m | s << 7;
    case GM_MFMASCAN_ENC_E2M3:
    case GM_MFMASCAN_ENC_E3M2: return m | s << 5;
    default: return m | s << 3;
  }
}

// The value of nibble n in half units: an integer in [-12, 12].
GM_CUSCAN_HD int32_t gm_mfmascan_half_units(uint32_t n) {
  const int32_t m = (int32_t)((0x0C08060403020100ull >> (8 * (n & 7u))) & 0xFFu);
  return n & 8u ? -m : m;
}

// ---- per-format geometry: elements per lane and operand (K = 4 times that), encoding, and
// whether the format carries E8M0 scales
GM_CUSCAN_HD int gm_mfmascan_elems(int f) {
  return f <= GM_MFMASCAN_IX_BF8 ? 8 : f == GM_MFMASCAN_IX_I8 ? 16 : f <= GM_MFMASCAN_IX_F64 ? 1 : 32;
}
GM_CUSCAN_HD int gm_mfmascan_enc(int f) {  // -1: not a nibble format
  switch (f) {
    case GM_MFMASCAN_IX_F16: return GM_MFMASCAN_ENC_F16;
    case GM_MFMASCAN_IX_FP8:
    case GM_MFMASCAN_IX_MXFP8: return GM_MFMASCAN_ENC_E4M3;
    case GM_MFMASCAN_IX_BF8:
    case GM_MFMASCAN_IX_MXBF8: return GM_MFMASCAN_ENC_E5M2;
    case GM_MFMASCAN_IX_MXFP6: return GM_MFMASCAN_ENC_E2M3;
    case GM_MFMASCAN_IX_MXBF6: return GM_MFMASCAN_ENC_E3M2;
    case GM_MFMASCAN_IX_MXFP4: return GM_MFMASCAN_ENC_E2M1;
    default: return -1;
  }
}
GM_CUSCAN_HD bool gm_mfmascan_scaled(int f) { return f >= GM_MFMASCAN_IX_MXFP8; }

// ---- hashes. q-th hash word of lane l's operand m (0: A, 1: B) of wave w in step s.
GM_CUSCAN_HD uint32_t gm_mfmascan_hash(uint64_t seed, int f, uint32_t s, uint32_t w, uint32_t m,
                                       uint32_t l, uint32_t q) {
  return gm_cuscan_hash(seed, GM_MFMASCAN_TEST_BASE + (uint32_t)f,
                        ((((s * 4 + w) * 2 + m) * 64 + l) * 4) + q);
}
// E8M0 scale byte of A's row (m = 0) or B's column (m = 1) r of wave w: 125..128, constant over
// the steps.
GM_CUSCAN_HD uint32_t gm_mfmascan_scale(uint64_t seed, int f, uint32_t w, uint32_t m, uint32_t r) {
  return 127u + (gm_cuscan_hash(seed, GM_MFMASCAN_SCALE_BASE + (uint32_t)f, (w * 2 + m) * 16 + r) &
                 3u) - 2u;
}
GM_CUSCAN_HD int32_t gm_mfmascan_f32_operand(uint32_t h) {
  return (int32_t)(h % (2u * GM_MFMASCAN_F32_MAX + 1u)) - GM_MFMASCAN_F32_MAX;
}
GM_CUSCAN_HD int32_t gm_mfmascan_f64_operand(uint32_t h) {  // [-2^22, 2^22)
  return (int32_t)(h & (2u * GM_MFMASCAN_F64_MAX - 1u)) - GM_MFMASCAN_F64_MAX;
}

// ---- register images. Nibble j of a hash word is element j of the 8 it feeds.
// dword of the 4 8-bit codes of nibbles 4 half .. 4 half + 3
GM_CUSCAN_HD uint32_t gm_mfmascan_pack8(int enc, uint32_t h, int half) {
  uint32_t d = 0;
  for (int j = 0; j < 4; ++j) d |= gm_mfmascan_code(enc, (h >> (16 * half + 4 * j)) & 15u) << (8 * j);
  return d;
}
// the 48 bits of the 8 6-bit codes of a hash word
GM_CUSCAN_HD uint64_t gm_mfmascan_pack6(int enc, uint32_t h) {
  uint64_t v = 0;
  for (int j = 0; j < 8; ++j) v |= (uint64_t)gm_mfmascan_code(enc, (h >> (4 * j)) & 15u) << (6 * j);
  return v;
}

// The operand image of lane l: the dwords the instruction reads, in register order; what a
// format does not use is zero. F is a GM_MFMASCAN_IX_* index.
//   f16            4 dwords, element e = half word e
//   fp8, bf8       2 dwords, element e = byte e
//   i8             4 dwords = 4 hash words, element e = byte e (signed)
//   f32, f64       the value's bit pattern (f64: low dword first)
//   mxfp8, mxbf8   8 dwords, element e = byte e, hash word e >> 3
//   mxfp6, mxbf6   6 dwords, element e = bits [6 e, 6 e + 6) of their 192-bit little-endian string
//   mxfp4          4 dwords = 4 hash words, element e = nibble e
template <int F>
GM_CUSCAN_HD void gm_mfmascan_image(uint64_t seed, uint32_t s, uint32_t w, uint32_t m, uint32_t l,
                                    uint32_t img[8]) {
  for (int i = 0; i < 8; ++i) img[i] = 0;
  const uint32_t h0 = gm_mfmascan_hash(seed, F, s, w, m, l, 0);
  if constexpr (F == GM_MFMASCAN_IX_F16) {
    for (int j = 0; j < 8; ++j)
      img[j >> 1] |= gm_mfmascan_code(GM_MFMASCAN_ENC_F16, (h0 >> (4 * j)) & 15u) << (16 * (j & 1));
  } else if constexpr (F == GM_MFMASCAN_IX_FP8 || F == GM_MFMASCAN_IX_BF8) {
    img[0] = gm_mfmascan_pack8(gm_mfmascan_enc(F), h0, 0);
    img[1] = gm_mfmascan_pack8(gm_mfmascan_enc(F), h0, 1);
  } else if constexpr (F == GM_MFMASCAN_IX_F32) {
    img[0] = gm_cuscan_f32_bits((float)gm_mfmascan_f32_operand(h0));
  } else if constexpr (F == GM_MFMASCAN_IX_F64) {
    const double d = (double)gm_mfmascan_f64_operand(h0);
    uint64_t u;
    __builtin_memcpy(&u, &d, 8);
    img[0] = (uint32_t)u;
    img[1] = (uint32_t)(u >> 32);
  } else {
    const uint32_t h[4] = {h0, gm_mfmascan_hash(seed, F, s, w, m, l, 1),
                           gm_mfmascan_hash(seed, F, s, w, m, l, 2),
                           gm_mfmascan_hash(seed, F, s, w, m, l, 3)};
    if constexpr (F == GM_MFMASCAN_IX_I8 || F == GM_MFMASCAN_IX_MXFP4) {
      for (int q = 0; q < 4; ++q) img[q] = h[q];
    } else if constexpr (F == GM_MFMASCAN_IX_MXFP8 || F == GM_MFMASCAN_IX_MXBF8) {
      for (int q = 0; q < 4; ++q) {
        img[2 * q] = gm_mfmascan_pack8(gm_mfmascan_enc(F), h[q], 0);
        img[2 * q + 1] = gm_mfmascan_pack8(gm_mfmascan_enc(F), h[q], 1);
      }
    } else {  // mxfp6, mxbf6: four 48-bit groups end to end
      const uint64_t v0 = gm_mfmascan_pack6(gm_mfmascan_enc(F), h[0]),
                     v1 = gm_mfmascan_pack6(gm_mfmascan_enc(F), h[1]),
                     v2 = gm_mfmascan_pack6(gm_mfmascan_enc(F), h[2]),
                     v3 = gm_mfmascan_pack6(gm_mfmascan_enc(F), h[3]);
      const uint64_t w0 = v0 | v1 << 48, w1 = v1 >> 16 | v2 << 32, w2 = v2 >> 32 | v3 << 16;
      img[0] = (uint32_t)w0;
      img[1] = (uint32_t)(w0 >> 32);
      img[2] = (uint32_t)w1;
      img[3] = (uint32_t)(w1 >> 32);
      img[4] = (uint32_t)w2;
      img[5] = (uint32_t)(w2 >> 32);
    }
  }
}

// The signature word of an f64 accumulator.
GM_CUSCAN_HD uint32_t gm_mfmascan_f64_word(double d) {
  uint64_t u;
  __builtin_memcpy(&u, &d, 8);
  return (uint32_t)u ^ gm_cuscan_rotl32((uint32_t)(u >> 32), 16);
}

// ------------------------------------------------------------------------------ host only
inline void gm_mfmascan_image_host(int f, uint64_t seed, uint32_t s, uint32_t w, uint32_t m,
                                   uint32_t l, uint32_t img[8]) {
  switch (f) {
#define GM_MFMASCAN_CASE(F) \
  case F: gm_mfmascan_image<F>(seed, s, w, m, l, img); break;
    GM_MFMASCAN_CASE(0) GM_MFMASCAN_CASE(1) GM_MFMASCAN_CASE(2) GM_MFMASCAN_CASE(3)
    GM_MFMASCAN_CASE(4) GM_MFMASCAN_CASE(5) GM_MFMASCAN_CASE(6) GM_MFMASCAN_CASE(7)
    GM_MFMASCAN_CASE(8) GM_MFMASCAN_CASE(9) GM_MFMASCAN_CASE(10)
#undef GM_MFMASCAN_CASE
    default: for (int i = 0; i < 8; ++i) img[i] = 0;
  }
}

// bits [pos, pos + width) of an image, width <= 16
inline uint32_t gm_mfmascan_bits(const uint32_t img[8], int pos, int width) {
  uint64_t v = img[pos >> 5];
  if ((pos >> 5) + 1 < 8) v |= (uint64_t)img[(pos >> 5) + 1] << 32;
  return (uint32_t)(v >> (pos & 31)) & ((1u << width) - 1u);
}

// Element e of an image as an integer: the value itself (i8, f32, f64), or the value in half
// units (nibble formats), read back from the image by the format's packing and code table.
inline int64_t gm_mfmascan_element_host(int f, const uint32_t img[8], int e) {
  if (f == GM_MFMASCAN_IX_I8) return (int8_t)gm_mfmascan_bits(img, 8 * e, 8);
  if (f == GM_MFMASCAN_IX_F32) {
    float v;
    __builtin_memcpy(&v, &img[0], 4);
    return (int64_t)v;
  }
  if (f == GM_MFMASCAN_IX_F64) {
    double v;
    __builtin_memcpy(&v, &img[0], 8);
    return (int64_t)v;
  }
  const int enc = gm_mfmascan_enc(f);
  const int width = enc == GM_MFMASCAN_ENC_F16 ? 16 : enc <= GM_MFMASCAN_ENC_E5M2 ? 8
                    : enc <= GM_MFMASCAN_ENC_E3M2 ? 6 : 4;
  const uint32_t code = gm_mfmascan_bits(img, width * e, width);
  for (uint32_t n = 0; n < 16; ++n)
    if (gm_mfmascan_code(enc, n) == code) return gm_mfmascan_half_units(n);
  return INT64_MIN;  // not a code of the table: cannot happen for an image built above
}

// The expected table of a whole block, out[4 t + i], for one format bit and 1 <= iters <=
// GM_MFMASCAN_MAX_ITERS (the entry points check both). Written over register images:
//   C[i][j] = sum over h < 4, e of a(lane i + 16 h, e) * b(lane j + 16 h, e)
// which holds for any instruction whose lane l carries row (A) / column (B) l & 15 and in which
// element e of K-group l >> 4 names the same k in A and in B.
inline void gm_mfmascan_expected_host(uint32_t format, uint64_t seed, uint32_t iters,
                                      uint32_t out[GM_CUSCAN_SIG_WORDS]) {
  const int f = __builtin_ctz(format);
  const int elems = gm_mfmascan_elems(f);
  const bool nibble = gm_mfmascan_enc(f) >= 0;
  for (uint32_t w = 0; w < 4; ++w) {
    int64_t c[16][16] = {};
    for (uint32_t s = 0; s < iters; ++s) {
      int64_t a[64][32], b[64][32];
      for (uint32_t l = 0; l < 64; ++l) {
        uint32_t ia[8], ib[8];
        gm_mfmascan_image_host(f, seed, s, w, 0, l, ia);
        gm_mfmascan_image_host(f, seed, s, w, 1, l, ib);
        for (int e = 0; e < elems; ++e) {
          a[l][e] = gm_mfmascan_element_host(f, ia, e);
          b[l][e] = gm_mfmascan_element_host(f, ib, e);
        }
      }
      for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j)
          for (int h = 0; h < 4; ++h)
            for (int e = 0; e < elems; ++e) c[i][j] += a[i + 16 * h][e] * b[j + 16 * h][e];
    }
    for (uint32_t l = 0; l < 64; ++l)
      for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t col = l & 15;
        const uint32_t row = f == GM_MFMASCAN_IX_F64 ? (l >> 4) + 4 * r : 4 * (l >> 4) + r;
        const int64_t q = c[row][col];
        uint32_t word;
        if (f == GM_MFMASCAN_IX_I8) {
          word = (uint32_t)(int32_t)q;
        } else if (f == GM_MFMASCAN_IX_F64) {
          word = gm_mfmascan_f64_word((double)q);
        } else if (!nibble) {
          word = gm_cuscan_f32_bits((float)q);
        } else {
          // q counts quarters; a sum of zero is +0.0
          int exp2 = -2;
          if (gm_mfmascan_scaled(f))
            exp2 += (int)gm_mfmascan_scale(seed, f, w, 0, row) +
                    (int)gm_mfmascan_scale(seed, f, w, 1, col) - 254;
          word = gm_cuscan_f32_bits(__builtin_ldexpf((float)q, exp2));
        }
        out[(w * 64 + l) * 4 + r] = word;
      }
  }
}
