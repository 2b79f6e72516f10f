// gm_sparsescan_ref.h — the sparse (2:4) and 32x32 matrix-core scan's value model: format bits,
// caps, the bf16 code table, the operand register images and index words (one definition for the
// host and for the gfx950 kernel, native/hip/gm_sparsescan.hip), the sparse operand model and
// the host evaluation of a block's expected table.
// The formulas and the premises are written out in gm_probe.h; this is their only implementation.
//
// The values are the format scan's (gm_mfmascan_ref.h): the sixteen e2m1 values, held exactly by
// every encoding, so that each product and each partial sum is exact in the accumulator type and
// the result is one definite bit pattern in any summation order.
#pragma once
#include <stdint.h>

#include "gm_mfmascan_ref.h"

enum {
  GM_SPARSESCAN_F16 = 1,        // v_smfmac_f32_16x16x64_f16
  GM_SPARSESCAN_BF16 = 2,       // v_smfmac_f32_16x16x64_bf16
  GM_SPARSESCAN_I8 = 4,         // v_smfmac_i32_16x16x128_i8
  GM_SPARSESCAN_FP8 = 8,        // v_smfmac_f32_16x16x128_fp8_fp8 (OCP e4m3)
  GM_SPARSESCAN_BF8 = 16,       // v_smfmac_f32_16x16x128_bf8_bf8 (e5m2)
  GM_SPARSESCAN_FP8BF8 = 32,    // v_smfmac_f32_16x16x128_fp8_bf8 (A e4m3, B e5m2)
  GM_SPARSESCAN_BF8FP8 = 64,    // v_smfmac_f32_16x16x128_bf8_fp8 (A e5m2, B e4m3)
  GM_SPARSESCAN_F16_32 = 128,   // v_smfmac_f32_32x32x32_f16
  GM_SPARSESCAN_BF16_32 = 256,  // v_smfmac_f32_32x32x32_bf16
  GM_SPARSESCAN_I8_32 = 512,    // v_smfmac_i32_32x32x64_i8
  GM_SPARSESCAN_FP8_32 = 1024,  // v_smfmac_f32_32x32x64_fp8_fp8
  GM_SPARSESCAN_ALL = 2047,
};

#define GM_SPARSESCAN_FORMATS 11
#define GM_SPARSESCAN_DEFAULT_ITERS 16
#define GM_SPARSESCAN_MAX_ITERS 63
#define GM_SPARSESCAN_TEST_BASE 0x700u  /* hash test ids: disjoint from every other scan's and */
#define GM_SPARSESCAN_INDEX_BASE 0x720u /* test's (1..0x6ff; the format scan's are 0x200..0x23f) */
#define GM_SPARSESCAN_A_DWORDS 4
#define GM_SPARSESCAN_B_DWORDS 8
#define GM_SPARSESCAN_ACC_WORDS 16      /* raw accumulator registers of a 32x32 form */

// Format indices: bit = 1 << index.
enum {
  GM_SPARSESCAN_IX_F16, GM_SPARSESCAN_IX_BF16, GM_SPARSESCAN_IX_I8, GM_SPARSESCAN_IX_FP8,
  GM_SPARSESCAN_IX_BF8, GM_SPARSESCAN_IX_FP8BF8, GM_SPARSESCAN_IX_BF8FP8,
  GM_SPARSESCAN_IX_F16_32, GM_SPARSESCAN_IX_BF16_32, GM_SPARSESCAN_IX_I8_32,
  GM_SPARSESCAN_IX_FP8_32,
};

// One more element encoding than the format scan's: bf16.
#define GM_SPARSESCAN_ENC_BF16 GM_MFMASCAN_ENCODINGS

// ---- caps. An output sums at most 64 kept products per step (K = 128 dense, half of it kept).
static_assert(GM_SPARSESCAN_MAX_ITERS == GM_MFMASCAN_MAX_ITERS, "one cap for both scans");
static_assert((uint64_t)GM_MFMASCAN_NIBBLE_MAX_PRODUCT * 64 * GM_SPARSESCAN_MAX_ITERS < (1ull << 24),
              "nibble forms: 144 quarter units x 64 kept products x iters is an exact fp32");
static_assert(128ull * 128 * 64 * GM_SPARSESCAN_MAX_ITERS < (1ull << 31),
              "i8: |product| <= 2^14, 64 kept products per step: the sum stays inside an int32");

// ---- code tables: the format scan's, and bf16 for the same sixteen values. A bf16 code is the
// upper half word of the value's fp32 pattern: 0, 1/2, 1, 3/2, 2, 3, 4, 6.
GM_CUSCAN_HD uint32_t gm_sparsescan_code(int enc, uint32_t n) {
  if (enc != GM_SPARSESCAN_ENC_BF16) return gm_mfmascan_code(enc, n);
  const uint64_t hi = 0x404040403F3F3F00ull, lo = 0xC0804000C0800000ull;  // byte n & 7 of each
  const uint32_t s = 8 * (n & 7u);
  return ((uint32_t)(hi >> s) & 0xFFu) << 8 | ((uint32_t)(lo >> s) & 0xFFu) | (n & 8u) << 12;
}

// ---- per-format geometry
GM_CUSCAN_HD bool gm_sparsescan_big(int f) { return f >= GM_SPARSESCAN_IX_F16_32; }  // 32x32
GM_CUSCAN_HD bool gm_sparsescan_wide(int f) {  // 16-bit elements
  return f == GM_SPARSESCAN_IX_F16 || f == GM_SPARSESCAN_IX_BF16 ||
         f == GM_SPARSESCAN_IX_F16_32 || f == GM_SPARSESCAN_IX_BF16_32;
}
GM_CUSCAN_HD bool gm_sparsescan_int(int f) {
  return f == GM_SPARSESCAN_IX_I8 || f == GM_SPARSESCAN_IX_I8_32;
}
// dense groups of four per lane: 4 (16-bit forms) or 8; kept elements 2 per group, dense 4
GM_CUSCAN_HD int gm_sparsescan_groups(int f) { return gm_sparsescan_wide(f) ? 4 : 8; }
// the encoding of operand m (0: A, 1: B); -1: raw bytes (i8)
GM_CUSCAN_HD int gm_sparsescan_enc(int f, int m) {
  switch (f) {
    case GM_SPARSESCAN_IX_F16:
    case GM_SPARSESCAN_IX_F16_32: return GM_MFMASCAN_ENC_F16;
    case GM_SPARSESCAN_IX_BF16:
    case GM_SPARSESCAN_IX_BF16_32: return GM_SPARSESCAN_ENC_BF16;
    case GM_SPARSESCAN_IX_FP8:
    case GM_SPARSESCAN_IX_FP8_32: return GM_MFMASCAN_ENC_E4M3;
    case GM_SPARSESCAN_IX_BF8: return GM_MFMASCAN_ENC_E5M2;
    case GM_SPARSESCAN_IX_FP8BF8: return m == 0 ? GM_MFMASCAN_ENC_E4M3 : GM_MFMASCAN_ENC_E5M2;
    case GM_SPARSESCAN_IX_BF8FP8: return m == 0 ? GM_MFMASCAN_ENC_E5M2 : GM_MFMASCAN_ENC_E4M3;
    default: return -1;
  }
}
// which half of the index register a step of a 16-bit form uses; the 8-bit forms use all of it
GM_CUSCAN_HD uint32_t gm_sparsescan_abid(int f, uint32_t s) {
  return gm_sparsescan_wide(f) ? s & 1u : 0u;
}

// ---- hashes. q-th hash word (q < 8) of lane l's operand m (0: A, 1: B) of wave w in step s.
GM_CUSCAN_HD uint32_t gm_sparsescan_hash(uint64_t seed, int f, uint32_t s, uint32_t w, uint32_t m,
                                         uint32_t l, uint32_t q) {
  return gm_cuscan_hash(seed, GM_SPARSESCAN_TEST_BASE + (uint32_t)f,
                        ((((s * 4 + w) * 2 + m) * 64 + l) * 8) + q);
}
// The nibble [i0 | i1 << 2] of one of the six ordered pairs i0 < i1:
// (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).
GM_CUSCAN_HD uint32_t gm_sparsescan_pair(uint32_t p) { return (0xED9C84u >> (4 * p)) & 15u; }
// The index register of lane l: nibble j is the pair of hash j % 6. An 8-bit form's nibble j is
// group j; a 16-bit form's is group j & 3 of set j >> 2.
GM_CUSCAN_HD uint32_t gm_sparsescan_index(uint64_t seed, int f, uint32_t s, uint32_t w, uint32_t l) {
  uint32_t idx = 0;
  for (uint32_t j = 0; j < 8; ++j)
    idx |= gm_sparsescan_pair(gm_cuscan_hash(seed, GM_SPARSESCAN_INDEX_BASE + (uint32_t)f,
                                             (((s * 4 + w) * 64 + l) * 8) + j) % 6u)
           << (4 * j);
  return idx;
}

// dword d of an operand of 16-bit codes: nibbles 2 (d & 3), 2 (d & 3) + 1 of hash word d >> 2
GM_CUSCAN_HD uint32_t gm_sparsescan_pack16(int enc, uint32_t h, int d) {
  return gm_sparsescan_code(enc, (h >> (8 * (d & 3))) & 15u) |
         gm_sparsescan_code(enc, (h >> (8 * (d & 3) + 4)) & 15u) << 16;
}

// The images of lane l in step s: the dwords the instruction reads, in register order.
//   A: 4 dwords, the kept elements. 16-bit forms: 8 half words, nibbles of hash word 0.
//      8-bit nibble forms: 16 bytes, nibbles of hash words 0, 1. i8: hash words 0..3.
//   B: 8 dwords, dense. 16-bit forms: 16 half words, nibbles of hash words 0, 1.
//      8-bit nibble forms: 32 bytes, nibbles of hash words 0..3. i8: hash words 0..7.
// Element e is nibble e & 7 of hash word e >> 3 and sits at bits [width e, width (e + 1)).
template <int F>
GM_CUSCAN_HD void gm_sparsescan_images(uint64_t seed, uint32_t s, uint32_t w, uint32_t l,
                                       uint32_t a[GM_SPARSESCAN_A_DWORDS],
                                       uint32_t b[GM_SPARSESCAN_B_DWORDS], uint32_t& idx) {
  idx = gm_sparsescan_index(seed, F, s, w, l);
  if constexpr (F == GM_SPARSESCAN_IX_I8 || F == GM_SPARSESCAN_IX_I8_32) {
    for (int d = 0; d < 4; ++d) a[d] = gm_sparsescan_hash(seed, F, s, w, 0, l, d);
    for (int d = 0; d < 8; ++d) b[d] = gm_sparsescan_hash(seed, F, s, w, 1, l, d);
  } else if constexpr (F == GM_SPARSESCAN_IX_F16 || F == GM_SPARSESCAN_IX_BF16 ||
                       F == GM_SPARSESCAN_IX_F16_32 || F == GM_SPARSESCAN_IX_BF16_32) {
    const uint32_t ha = gm_sparsescan_hash(seed, F, s, w, 0, l, 0);
    const uint32_t hb[2] = {gm_sparsescan_hash(seed, F, s, w, 1, l, 0),
                            gm_sparsescan_hash(seed, F, s, w, 1, l, 1)};
    for (int d = 0; d < 4; ++d) a[d] = gm_sparsescan_pack16(gm_sparsescan_enc(F, 0), ha, d);
    for (int d = 0; d < 8; ++d) b[d] = gm_sparsescan_pack16(gm_sparsescan_enc(F, 1), hb[d >> 2], d);
  } else {
    for (int q = 0; q < 2; ++q) {
      const uint32_t h = gm_sparsescan_hash(seed, F, s, w, 0, l, q);
      a[2 * q] = gm_mfmascan_pack8(gm_sparsescan_enc(F, 0), h, 0);
      a[2 * q + 1] = gm_mfmascan_pack8(gm_sparsescan_enc(F, 0), h, 1);
    }
    for (int q = 0; q < 4; ++q) {
      const uint32_t h = gm_sparsescan_hash(seed, F, s, w, 1, l, q);
      b[2 * q] = gm_mfmascan_pack8(gm_sparsescan_enc(F, 1), h, 0);
      b[2 * q + 1] = gm_mfmascan_pack8(gm_sparsescan_enc(F, 1), h, 1);
    }
  }
}

// Word i of a 32x32 form's signature: the fold of accumulator registers 4 i .. 4 i + 3.
GM_CUSCAN_HD uint32_t gm_sparsescan_fold(const uint32_t bits[4]) {
  uint32_t x = 0;
  for (int j = 0; j < 4; ++j) x = gm_cuscan_rotl32(x, 5) + bits[j];
  return x;
}

// ------------------------------------------------------------------------------ host only
inline void gm_sparsescan_images_host(int f, uint64_t seed, uint32_t s, uint32_t w, uint32_t l,
                                      uint32_t a[GM_SPARSESCAN_A_DWORDS],
                                      uint32_t b[GM_SPARSESCAN_B_DWORDS], uint32_t& idx) {
  switch (f) {
#define GM_SPARSESCAN_CASE(F) \
  case F: gm_sparsescan_images<F>(seed, s, w, l, a, b, idx); break;
    GM_SPARSESCAN_CASE(0) GM_SPARSESCAN_CASE(1) GM_SPARSESCAN_CASE(2) GM_SPARSESCAN_CASE(3)
    GM_SPARSESCAN_CASE(4) GM_SPARSESCAN_CASE(5) GM_SPARSESCAN_CASE(6) GM_SPARSESCAN_CASE(7)
    GM_SPARSESCAN_CASE(8) GM_SPARSESCAN_CASE(9) GM_SPARSESCAN_CASE(10)
#undef GM_SPARSESCAN_CASE
    default:
      for (int i = 0; i < GM_SPARSESCAN_A_DWORDS; ++i) a[i] = 0;
      for (int i = 0; i < GM_SPARSESCAN_B_DWORDS; ++i) b[i] = 0;
      idx = 0;
  }
}

// Element e of operand m's image as an integer: the byte (i8), or the value in half units read
// back from the image by the format's code table. INT64_MIN: not a code of the table.
inline int64_t gm_sparsescan_element_host(int f, int m, const uint32_t* img, int e) {
  const int width = gm_sparsescan_wide(f) ? 16 : 8;
  const uint32_t code = (img[(width * e) >> 5] >> ((width * e) & 31)) & ((1u << width) - 1u);
  if (gm_sparsescan_int(f)) return (int8_t)code;
  const int enc = gm_sparsescan_enc(f, m);
  for (uint32_t n = 0; n < 16; ++n)
    if (gm_sparsescan_code(enc, n) == code) return gm_mfmascan_half_units(n);
  return INT64_MIN;
}

// Position p (0, 1) of dense group g in index register idx with set selector abid.
inline int gm_sparsescan_position(int f, uint32_t idx, uint32_t abid, int g, int p) {
  const uint32_t set = gm_sparsescan_wide(f) ? (idx >> (16 * (abid & 1u))) & 0xFFFFu : idx;
  return (int)((set >> (4 * g + 2 * p)) & 3u);
}

// The sparse operand model: lane l's A image expanded to the dense elements of its K-group
// (4 * groups of them). Kept elements 2 g and 2 g + 1 belong to dense group g and sit at dense
// positions 4 g + i0 and 4 g + i1; every other position is zero. With i0 == i1 (which the scan
// never issues) the later element would overwrite the earlier.
inline void gm_sparsescan_expand_host(int f, const uint32_t a[GM_SPARSESCAN_A_DWORDS],
                                      uint32_t idx, uint32_t abid, int64_t dense[32]) {
  for (int e = 0; e < 32; ++e) dense[e] = 0;
  for (int g = 0; g < gm_sparsescan_groups(f); ++g)
    for (int p = 0; p < 2; ++p)
      dense[4 * g + gm_sparsescan_position(f, idx, abid, g, p)] =
          gm_sparsescan_element_host(f, 0, a, 2 * g + p);
}

// Row of a lane's accumulator register r, and its column: the C/D maps of the two shapes.
inline int gm_sparsescan_row(int f, uint32_t l, int r) {
  return gm_sparsescan_big(f) ? 8 * (r >> 2) + 4 * (int)(l >> 5) + (r & 3) : 4 * (int)(l >> 4) + r;
}
inline int gm_sparsescan_col(int f, uint32_t l) { return (int)(l & (gm_sparsescan_big(f) ? 31u : 15u)); }

// The k that dense element e of K-group h names, K-groups = 4 (16x16) or 2 (32x32), D = dense
// elements per lane. A's dense expansion is contiguous: k = D h + e. B is laid out as two
// instructions of half the K side by side: its element e is k = (K / 2) (e / (D / 2)) +
// (D / 2) h + e % (D / 2). (Read off the hardware with one-hot operands; the dense format scan
// cannot see this, there A and B follow one rule.)
inline int gm_sparsescan_k_a(int f, int h, int e) { return 4 * gm_sparsescan_groups(f) * h + e; }
inline int gm_sparsescan_k_b(int f, int h, int e) {
  const int half = 2 * gm_sparsescan_groups(f), kgroups = gm_sparsescan_big(f) ? 2 : 4;
  return half * kgroups * (e / half) + half * h + e % half;
}

// One instruction of one wave on register images, added to c (integers: i8 the value, nibble
// forms quarter units):
//   c[i][j] += sum over k of A[i][k] * B[k][j],  A[l & (R - 1)][k_a(l / R, e)] = dense_a(l, e),
//                                                B[k_b(l / R, e)][l & (R - 1)] = b(l, e)
// with R = 16 rows and 4 K-groups, or 32 and 2.
inline void gm_sparsescan_accumulate_host(int f, const uint32_t* a /*[64][4]*/,
                                          const uint32_t* b /*[64][8]*/,
                                          const uint32_t* idx /*[64]*/, uint32_t abid,
                                          int64_t c[32][32]) {
  const int R = gm_sparsescan_big(f) ? 32 : 16;
  const int dense_per_lane = 4 * gm_sparsescan_groups(f), K = dense_per_lane * (64 / R);
  int64_t am[32][128], bm[128][32];
  for (int l = 0; l < 64; ++l) {
    int64_t dense[32];
    gm_sparsescan_expand_host(f, a + l * GM_SPARSESCAN_A_DWORDS, idx[l], abid, dense);
    for (int e = 0; e < dense_per_lane; ++e) {
      am[l % R][gm_sparsescan_k_a(f, l / R, e)] = dense[e];
      bm[gm_sparsescan_k_b(f, l / R, e)][l % R] =
          gm_sparsescan_element_host(f, 1, b + l * GM_SPARSESCAN_B_DWORDS, e);
    }
  }
  for (int i = 0; i < R; ++i)
    for (int j = 0; j < R; ++j)
      for (int k = 0; k < K; ++k) c[i][j] += am[i][k] * bm[k][j];
}

// The bit pattern of an accumulator that holds q (i8: the int32; else q quarter units as fp32,
// a sum of zero being +0.0).
inline uint32_t gm_sparsescan_acc_bits(int f, int64_t q) {
  return gm_sparsescan_int(f) ? (uint32_t)(int32_t)q
                              : gm_cuscan_f32_bits(__builtin_ldexpf((float)q, -2));
}

// The 16 raw accumulator registers of every lane of one wave (a 16x16 form: 4, the rest zero).
inline void gm_sparsescan_acc_host(int f, const int64_t c[32][32],
                                   uint32_t out[64 * GM_SPARSESCAN_ACC_WORDS]) {
  const int regs = gm_sparsescan_big(f) ? 16 : 4;
  for (uint32_t l = 0; l < 64; ++l)
    for (int r = 0; r < GM_SPARSESCAN_ACC_WORDS; ++r)
      out[l * GM_SPARSESCAN_ACC_WORDS + r] =
          r < regs ? gm_sparsescan_acc_bits(
                         f, c[gm_sparsescan_row(f, l, r)][gm_sparsescan_col(f, l)])
                   : 0u;
}

// The expected table of a whole block, out[4 t + i], for one format bit and 1 <= iters <=
// GM_SPARSESCAN_MAX_ITERS (the entry points check both), from the register images of every step.
inline void gm_sparsescan_expected_host(uint32_t format, uint64_t seed, uint32_t iters,
                                        uint32_t out[GM_CUSCAN_SIG_WORDS]) {
  const int f = __builtin_ctz(format);
  for (uint32_t w = 0; w < 4; ++w) {
    int64_t c[32][32] = {};
    for (uint32_t s = 0; s < iters; ++s) {
      uint32_t a[64 * GM_SPARSESCAN_A_DWORDS], b[64 * GM_SPARSESCAN_B_DWORDS], idx[64];
      for (uint32_t l = 0; l < 64; ++l)
        gm_sparsescan_images_host(f, seed, s, w, l, a + l * GM_SPARSESCAN_A_DWORDS,
                                  b + l * GM_SPARSESCAN_B_DWORDS, idx[l]);
      gm_sparsescan_accumulate_host(f, a, b, idx, gm_sparsescan_abid(f, s), c);
    }
    uint32_t acc[64 * GM_SPARSESCAN_ACC_WORDS];
    gm_sparsescan_acc_host(f, c, acc);
    for (uint32_t l = 0; l < 64; ++l)
      for (uint32_t i = 0; i < 4; ++i)
        out[(w * 64 + l) * 4 + i] =
            gm_sparsescan_big(f) ? gm_sparsescan_fold(acc + l * GM_SPARSESCAN_ACC_WORDS + 4 * i)
                                 : acc[l * GM_SPARSESCAN_ACC_WORDS + i];
  }
}
