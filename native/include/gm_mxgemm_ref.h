// gm_mxgemm_ref.h — the block-scaled (MX) GEMM burn-in's value model: the operand fills (one
// definition for the host and for the gfx950 fill kernel, native/hip/gm_mxgemm.hip), the decoders
// and the host evaluation of the expected result. The formulas are written out in gm_probe.h;
// this is their only implementation.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "gm_mfmascan_ref.h"

// Formats: the number is the instruction's cbsz / blgp format field.
enum { GM_MX_FP8 = 0, GM_MX_FP4 = 4 };
// Operand classes.
enum { GM_MX_EXACT = 0, GM_MX_BLOCKS = 1, GM_MX_RANDOM = 2, GM_MX_CLASSES = 3 };

#define GM_MX_BLOCK 32               /* elements that share one E8M0 scale */
#define GM_MX_SCALE_SALT 0x5CA1E5CAu /* a scale's hash uses seed ^ this */

GM_CUSCAN_HD bool gm_mx_format_ok(int fmt) { return fmt == GM_MX_FP8 || fmt == GM_MX_FP4; }
GM_CUSCAN_HD bool gm_mx_class_ok(int cls) { return cls >= 0 && cls < GM_MX_CLASSES; }
// Elements of one K-tile of the kernel (128 bytes of a row) and bytes of a row of K elements.
GM_CUSCAN_HD int gm_mx_tile_k(int fmt) { return fmt == GM_MX_FP4 ? 256 : 128; }
GM_CUSCAN_HD size_t gm_mx_row_bytes(int fmt, size_t k) { return fmt == GM_MX_FP4 ? k / 2 : k; }

// The burn-in fill's hash (gm_probe_fill_bf16's), of a 32-bit index.
GM_CUSCAN_HD uint32_t gm_mx_hash(uint32_t i, uint32_t seed) {
  uint32_t h = i * 2654435761u ^ seed;
  h ^= h >> 15;
  h *= 2246822519u;
  h ^= h >> 13;
  return h;
}

// The code of element e (= row * K + k) of an operand: a nibble (fp4) or an e4m3 byte (fp8).
GM_CUSCAN_HD uint32_t gm_mx_element(int fmt, int cls, uint32_t seed, uint64_t e) {
  const uint32_t h = gm_mx_hash((uint32_t)e, seed);
  if (cls == GM_MX_RANDOM && fmt == GM_MX_FP8) {
    uint32_t b = h >> 24;
    if ((b & 0x7Fu) == 0x7Fu) b = (b & 0x80u) | ((h >> 8) & 0x7Eu);  // never a NaN code
    return b;
  }
  // blocks: 0, 1, 2, -1, -2 as e2m1 nibbles 0, 2, 4, 10, 12; exact and random: any nibble
  const uint32_t n = cls == GM_MX_BLOCKS ? (0xCA420u >> (4 * ((h >> 8) % 5u))) & 15u : h >> 28;
  return fmt == GM_MX_FP4 ? n : gm_mfmascan_code(GM_MFMASCAN_ENC_E4M3, n);
}

// The E8M0 byte of row `row`, K-block `kb` of an operand with kblocks = K / 32 blocks per row.
GM_CUSCAN_HD uint32_t gm_mx_scale(int cls, uint32_t seed, uint32_t row, uint32_t kb,
                                  uint32_t kblocks) {
  const uint32_t s = seed ^ GM_MX_SCALE_SALT;
  if (cls == GM_MX_EXACT) return 125u + (gm_mx_hash(row, s) >> 30);
  const uint32_t h = gm_mx_hash(row * kblocks + kb, s);
  return cls == GM_MX_BLOCKS ? 127u + (h >> 31) : 123u + (h >> 29);
}

// Byte i of an operand's packed rows: one fp8 code, or fp4 elements 2 i (low nibble) and 2 i + 1.
GM_CUSCAN_HD uint32_t gm_mx_packed_byte(int fmt, int cls, uint32_t seed, uint64_t i) {
  if (fmt == GM_MX_FP8) return gm_mx_element(fmt, cls, seed, i);
  return gm_mx_element(fmt, cls, seed, 2 * i) | gm_mx_element(fmt, cls, seed, 2 * i + 1) << 4;
}

// ------------------------------------------------------------------------------ host only
// An e4m3 byte (OCP: bias 7, subnormals, no infinities; the caller feeds no NaN code).
inline double gm_mx_e4m3_value(uint32_t c) {
  const int e = (int)(c >> 3) & 15, m = (int)c & 7;
  const double v = e == 0 ? ldexp((double)m, -9) : ldexp((double)(8 + m), e - 10);
  return c & 0x80u ? -v : v;
}

inline double gm_mx_value(int fmt, uint32_t code) {
  return fmt == GM_MX_FP4 ? 0.5 * gm_mfmascan_half_units(code) : gm_mx_e4m3_value(code);
}

// The nibble an exact-class code stands for (fp8: through the code table).
inline uint32_t gm_mx_nibble_of(int fmt, uint32_t code) {
  if (fmt == GM_MX_FP4) return code;
  for (uint32_t n = 0; n < 16; ++n)
    if (gm_mfmascan_code(GM_MFMASCAN_ENC_E4M3, n) == code) return n;
  return 0;  // not a code of the table: cannot happen for the exact and blocks classes
}

// bf16 bits of v * 2^-6, rounded to nearest even; |v| < 2^53.
inline uint16_t gm_mx_bf16_of_units(int64_t v) {
  uint64_t a = v < 0 ? (uint64_t)(-v) : (uint64_t)v;
  if (a == 0) return 0;  // a sum of zero is +0.0
  int shift = 0;
  while ((a >> shift) >= 256) ++shift;
  if (shift) {
    const uint64_t rem = a & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    a >>= shift;
    if (rem > half || (rem == half && (a & 1))) ++a;  // 256 << shift is still 8 bits or fewer
    a <<= shift;
  }
  const float f = ldexpf((float)a, -6);
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return (uint16_t)((u >> 16) | (v < 0 ? 0x8000u : 0u));
}

// The expected result of C = A * Bt^T for operands filled with (fmt, cls, seed_a) and
// (fmt, cls, seed_b); K a multiple of 32.
//   exact, blocks: c[i * N + j] = the exact sum, rounded to bf16 (ref, abs_sum untouched);
//   random:        ref[i * N + j] = the float64 sum in k order, abs_sum[..] = sum of |product|
//                  (c untouched).
inline void gm_mxgemm_expected_host(int fmt, int cls, uint32_t seed_a, uint32_t seed_b, int M,
                                    int N, int K, uint16_t* c, double* ref, double* abs_sum) {
  const uint32_t kb = (uint32_t)K / GM_MX_BLOCK;
  if (cls != GM_MX_RANDOM) {
    // element * 2^(scale - 125) in units of 2^-3 (half units times four): scales are >= 125
    auto ints = [&](uint32_t seed, int rows) {
      std::vector<int32_t> v((size_t)rows * K);
      for (int r = 0; r < rows; ++r)
        for (int k = 0; k < K; ++k) {
          const uint32_t code = gm_mx_element(fmt, cls, seed, (uint64_t)r * K + k);
          const int sh = (int)gm_mx_scale(cls, seed, r, k / GM_MX_BLOCK, kb) - 125;
          v[(size_t)r * K + k] = gm_mfmascan_half_units(gm_mx_nibble_of(fmt, code)) * (1 << sh);
        }
      return v;
    };
    const std::vector<int32_t> a = ints(seed_a, M), b = ints(seed_b, N);
    for (int i = 0; i < M; ++i)
      for (int j = 0; j < N; ++j) {
        int64_t s = 0;
        for (int k = 0; k < K; ++k) s += (int64_t)a[(size_t)i * K + k] * b[(size_t)j * K + k];
        c[(size_t)i * N + j] = gm_mx_bf16_of_units(s);
      }
    return;
  }
  auto vals = [&](uint32_t seed, int rows) {
    std::vector<double> v((size_t)rows * K);
    for (int r = 0; r < rows; ++r)
      for (int k = 0; k < K; ++k)
        v[(size_t)r * K + k] =
            ldexp(gm_mx_value(fmt, gm_mx_element(fmt, cls, seed, (uint64_t)r * K + k)),
                  (int)gm_mx_scale(cls, seed, r, k / GM_MX_BLOCK, kb) - 127);
    return v;
  };
  const std::vector<double> a = vals(seed_a, M), b = vals(seed_b, N);
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < N; ++j) {
      double s = 0, t = 0;
      for (int k = 0; k < K; ++k) {
        const double p = a[(size_t)i * K + k] * b[(size_t)j * K + k];  // exact: 8 bits at most
        s += p;
        t += fabs(p);
      }
      ref[(size_t)i * N + j] = s;
      abs_sum[(size_t)i * N + j] = t;
    }
}
