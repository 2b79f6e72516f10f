// Host reference of the matrix-core format scan (include/gm_mfmascan_ref.h) under ASan/UBSan:
// the code tables against decoders written from the formats' definitions, the caps, and every
// format's table against a plain (row, k) x (k, column) triple loop.
// No GPU, no HIP, nothing loaded into an interpreter; part of `make -C native check`.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "gm_mfmascan_ref.h"

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                 \
    }                                                             \
  } while (0)

// sign, `ebits` exponent bits with bias `bias`, `mbits` mantissa bits; subnormals when the
// exponent field is 0. None of the codes in the tables is a NaN or an infinity of its format.
static double decode(uint32_t code, int ebits, int mbits, int bias) {
  const uint32_t m = code & ((1u << mbits) - 1u);
  const uint32_t e = (code >> mbits) & ((1u << ebits) - 1u);
  const double sign = (code >> (ebits + mbits)) & 1u ? -1.0 : 1.0;
  const double frac = (double)m / (double)(1u << mbits);
  return sign * (e == 0 ? ldexp(frac, 1 - bias) : ldexp(1.0 + frac, (int)e - bias));
}

static double decode_enc(int enc, uint32_t code) {
  switch (enc) {
    case GM_MFMASCAN_ENC_F16: return decode(code, 5, 10, 15);
    case GM_MFMASCAN_ENC_E4M3: return decode(code, 4, 3, 7);
    case GM_MFMASCAN_ENC_E5M2: return decode(code, 5, 2, 15);
    case GM_MFMASCAN_ENC_E2M3: return decode(code, 2, 3, 1);
    case GM_MFMASCAN_ENC_E3M2: return decode(code, 3, 2, 3);
    default: return decode(code, 2, 1, 1);
  }
}

static std::vector<uint32_t> table(uint32_t format, uint64_t seed, uint32_t iters) {
  std::vector<uint32_t> out(GM_CUSCAN_SIG_WORDS, 0xDEADBEEFu);
  gm_mfmascan_expected_host(format, seed, iters, out.data());
  return out;
}

// The same table from (row, k) matrices: lane l holds row / column l & 15 and the k values
// elems * (l >> 4) + e. (Any other k numbering common to A and B gives the same sums.)
static std::vector<uint32_t> triple_loop(int f, uint64_t seed, uint32_t iters) {
  const int elems = gm_mfmascan_elems(f), K = 4 * elems;
  const int enc = gm_mfmascan_enc(f);
  std::vector<uint32_t> out(GM_CUSCAN_SIG_WORDS);
  for (uint32_t w = 0; w < 4; ++w) {
    std::vector<double> c(256, 0.0);
    for (uint32_t s = 0; s < iters; ++s) {
      std::vector<double> a(16 * K), b(K * 16);
      for (uint32_t l = 0; l < 64; ++l)
        for (uint32_t m = 0; m < 2; ++m) {
          uint32_t img[8];
          gm_mfmascan_image_host(f, seed, s, w, m, l, img);
          for (int e = 0; e < elems; ++e) {
            double v;
            if (enc >= 0) {
              const int width = enc == GM_MFMASCAN_ENC_F16 ? 16 : enc <= GM_MFMASCAN_ENC_E5M2 ? 8
                                : enc <= GM_MFMASCAN_ENC_E3M2 ? 6 : 4;
              v = decode_enc(enc, gm_mfmascan_bits(img, width * e, width));
            } else {
              v = (double)gm_mfmascan_element_host(f, img, e);
            }
            const int k = elems * (int)(l >> 4) + e;
            if (m == 0) a[(l & 15) * K + k] = v;
            else b[k * 16 + (l & 15)] = v;
          }
        }
      for (int i = 0; i < 16; ++i)
        for (int k = 0; k < K; ++k)
          for (int j = 0; j < 16; ++j) c[i * 16 + j] += a[i * K + k] * b[k * 16 + j];
    }
    for (uint32_t l = 0; l < 64; ++l)
      for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t col = l & 15;
        const uint32_t row = f == GM_MFMASCAN_IX_F64 ? (l >> 4) + 4 * r : 4 * (l >> 4) + r;
        double v = c[row * 16 + col];
        if (gm_mfmascan_scaled(f))
          v = ldexp(v, (int)gm_mfmascan_scale(seed, f, w, 0, row) +
                           (int)gm_mfmascan_scale(seed, f, w, 1, col) - 254);
        if (v == 0.0) v = 0.0;  // +0
        uint32_t word;
        if (f == GM_MFMASCAN_IX_I8) word = (uint32_t)(int32_t)v;
        else if (f == GM_MFMASCAN_IX_F64) word = gm_mfmascan_f64_word(v);
        else word = gm_cuscan_f32_bits((float)v);
        out[(w * 64 + l) * 4 + r] = word;
      }
  }
  return out;
}

int main() {
  // each code table decodes to the e2m1 value set, and its codes are distinct
  const double mags[8] = {0, 0.5, 1, 1.5, 2, 3, 4, 6};
  for (int enc = 0; enc < GM_MFMASCAN_ENCODINGS; ++enc)
    for (uint32_t n = 0; n < 16; ++n) {
      const double v = decode_enc(enc, gm_mfmascan_code(enc, n));
      EXPECT(fabs(v) == mags[n & 7]);
      EXPECT(signbit(v) == ((n & 8) != 0));
      EXPECT(2 * v == (double)gm_mfmascan_half_units(n));
      for (uint32_t o = 0; o < n; ++o) EXPECT(gm_mfmascan_code(enc, o) != gm_mfmascan_code(enc, n));
    }
  EXPECT(gm_mfmascan_code(GM_MFMASCAN_ENC_E4M3, 7) == 0x4C);   // 6.0, not the 0x7F NaN
  EXPECT(gm_mfmascan_code(GM_MFMASCAN_ENC_F16, 10) == 0xBC00);  // -1.0

  // the caps at the largest accepted iters, and that f32's is the one that binds
  const uint64_t it = GM_MFMASCAN_MAX_ITERS;
  EXPECT(144ull * 128 * it < (1ull << 24));
  EXPECT(128ull * 128 * 64 * it < (1ull << 31));
  EXPECT(4ull * 255 * 255 * it < (1ull << 24));
  EXPECT(4ull * 255 * 255 * (it + 2) >= (1ull << 24));
  EXPECT(4ull * (1ull << 44) * it < (1ull << 53));
  for (uint32_t h = 0; h < 100000; h += 7) {
    EXPECT(abs(gm_mfmascan_f32_operand(h * 0x9E3779B1u)) <= GM_MFMASCAN_F32_MAX);
    EXPECT(abs(gm_mfmascan_f64_operand(h * 0x9E3779B1u)) <= GM_MFMASCAN_F64_MAX);
  }
  for (int f = GM_MFMASCAN_IX_MXFP8; f < GM_MFMASCAN_FORMATS; ++f)
    for (uint32_t i = 0; i < 128; ++i) {
      const uint32_t s = gm_mfmascan_scale(0x1234, f, i >> 5, (i >> 4) & 1, i & 15);
      EXPECT(s >= 125 && s <= 128);
    }

  // every format's table: a pure function of (seed, iters) that equals the triple loop
  const uint64_t seeds[2] = {0, 0x0123456789ABCDEFull};
  const uint32_t iters[2] = {1, 3};
  for (uint64_t seed : seeds)
    for (uint32_t n : iters)
      for (int f = 0; f < GM_MFMASCAN_FORMATS; ++f) {
        const std::vector<uint32_t> a = table(1u << f, seed, n);
        EXPECT(a == table(1u << f, seed, n));
        EXPECT(a != table(1u << f, seed ^ 1, n));
        EXPECT(a != table(1u << f, seed, n + 1));
        EXPECT(a == triple_loop(f, seed, n));
      }
  // and once at the cap
  EXPECT(table(GM_MFMASCAN_F32, 1, GM_MFMASCAN_MAX_ITERS) ==
         triple_loop(GM_MFMASCAN_IX_F32, 1, GM_MFMASCAN_MAX_ITERS));
  EXPECT(table(GM_MFMASCAN_MXFP6, 1, GM_MFMASCAN_MAX_ITERS) ==
         triple_loop(GM_MFMASCAN_IX_MXFP6, 1, GM_MFMASCAN_MAX_ITERS));

  if (failures) {
    printf("%d failure(s)\n", failures);
    return 1;
  }
  printf("test_mfmascan_host: ok\n");
  return 0;
}
