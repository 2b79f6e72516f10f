// Host side of the MX GEMM burn-in's value model (include/gm_mxgemm_ref.h) under ASan/UBSan:
// the fills against what gm_probe.h states about each class, the decoders against the formats'
// definitions, the bf16 rounding against the float conversion, and the expected results against
// a second, naive evaluation in floating point.
// No GPU, no HIP, nothing loaded into an interpreter; part of `make -C native check`.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <set>
#include <vector>

#include "gm_mxgemm_ref.h"

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                 \
    }                                                             \
  } while (0)

// sign, 4 exponent bits (bias 7), 3 mantissa bits, subnormals: OCP e4m3 from its definition
static double e4m3(uint32_t c) {
  const uint32_t m = c & 7u, e = (c >> 3) & 15u;
  const double v = e == 0 ? ldexp(m / 8.0, -6) : ldexp(1.0 + m / 8.0, (int)e - 7);
  return c & 0x80u ? -v : v;
}

static const double kE2m1[8] = {0, 0.5, 1, 1.5, 2, 3, 4, 6};

static uint16_t bf16_of_float(float f) {  // round to nearest even, finite input
  uint32_t u;
  memcpy(&u, &f, 4);
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

static void test_decoders() {
  for (uint32_t c = 0; c < 256; ++c)
    if ((c & 0x7Fu) != 0x7Fu) EXPECT(gm_mx_e4m3_value(c) == e4m3(c));
  EXPECT(gm_mx_e4m3_value(0x7E) == 448.0 && gm_mx_e4m3_value(0x01) == ldexp(1.0, -9));
  for (uint32_t n = 0; n < 16; ++n) {
    const double v = (n & 8u ? -1.0 : 1.0) * kE2m1[n & 7u];
    EXPECT(gm_mx_value(GM_MX_FP4, n) == v);
    const uint32_t code = gm_mfmascan_code(GM_MFMASCAN_ENC_E4M3, n);
    EXPECT(gm_mx_value(GM_MX_FP8, code) == v && gm_mx_nibble_of(GM_MX_FP8, code) == n);
    EXPECT(gm_mx_nibble_of(GM_MX_FP4, n) == n);
  }
  EXPECT(gm_mx_tile_k(GM_MX_FP8) == 128 && gm_mx_tile_k(GM_MX_FP4) == 256);
  EXPECT(gm_mx_row_bytes(GM_MX_FP8, 256) == 256 && gm_mx_row_bytes(GM_MX_FP4, 256) == 128);
  EXPECT(gm_mx_format_ok(0) && gm_mx_format_ok(4) && !gm_mx_format_ok(1) && !gm_mx_format_ok(-1));
  EXPECT(gm_mx_class_ok(0) && gm_mx_class_ok(2) && !gm_mx_class_ok(3) && !gm_mx_class_ok(-1));
}

static void test_rounding() {
  EXPECT(gm_mx_bf16_of_units(0) == 0);
  // every small integer, both signs; then values that need the rounding, among them exact ties
  for (int64_t v = -70000; v <= 70000; ++v)
    if (v) EXPECT(gm_mx_bf16_of_units(v) == bf16_of_float(ldexpf((float)v, -6)));
  const int64_t ties[] = {257, 258, 259, 383 << 1, 385 << 1, (255ll << 16) | 0x8000,
                          (255ll << 16) | 0x8001, (254ll << 16) | 0x8000, (1ll << 24) - 1,
                          (1ll << 24) - 128, 0xFF8000, 0xFF7FFF};
  for (int64_t t : ties)
    for (int64_t v : {t, -t}) EXPECT(gm_mx_bf16_of_units(v) == bf16_of_float(ldexpf((float)v, -6)));
  // beyond 24 bits the float conversion would round twice; the integer path rounds once
  EXPECT(gm_mx_bf16_of_units((1ll << 40) + (1ll << 32)) == bf16_of_float(ldexpf(1.0f, 34)));
  EXPECT(gm_mx_bf16_of_units((1ll << 40) + (1ll << 32) + 1) ==
         bf16_of_float(ldexpf(1.0f + 1.0f / 128, 34)));
}

static void test_fills() {
  const uint32_t seed = 0x5151u;
  const int rows = 64, K = 1024, kb = K / GM_MX_BLOCK;
  for (int fmt : {GM_MX_FP8, GM_MX_FP4}) {
    std::set<double> exact, blocks;
    std::set<uint32_t> random;
    for (uint64_t e = 0; e < (uint64_t)rows * K; ++e) {
      exact.insert(gm_mx_value(fmt, gm_mx_element(fmt, GM_MX_EXACT, seed, e)));
      blocks.insert(gm_mx_value(fmt, gm_mx_element(fmt, GM_MX_BLOCKS, seed, e)));
      const uint32_t c = gm_mx_element(fmt, GM_MX_RANDOM, seed, e);
      random.insert(c);
      EXPECT(fmt == GM_MX_FP4 ? c < 16 : c < 256 && (c & 0x7Fu) != 0x7Fu);
    }
    EXPECT(exact.size() == 15);  // -0 and +0 compare equal
    EXPECT(blocks == (std::set<double>{-2, -1, 0, 1, 2}));
    EXPECT(random.size() == (fmt == GM_MX_FP4 ? 16u : 254u));
    // packing: fp4 low nibble first
    for (uint64_t i = 0; i < 64; ++i) {
      const uint32_t b = gm_mx_packed_byte(fmt, GM_MX_EXACT, seed, i);
      if (fmt == GM_MX_FP4)
        EXPECT(b == (gm_mx_element(fmt, GM_MX_EXACT, seed, 2 * i) |
                     gm_mx_element(fmt, GM_MX_EXACT, seed, 2 * i + 1) << 4));
      else
        EXPECT(b == gm_mx_element(fmt, GM_MX_EXACT, seed, i));
    }
  }
  std::set<uint32_t> ex, bl, rnd;
  bool blocks_differ_along_k = false;
  for (uint32_t r = 0; r < (uint32_t)rows; ++r)
    for (uint32_t b = 0; b < (uint32_t)kb; ++b) {
      ex.insert(gm_mx_scale(GM_MX_EXACT, seed, r, b, kb));
      EXPECT(gm_mx_scale(GM_MX_EXACT, seed, r, b, kb) == gm_mx_scale(GM_MX_EXACT, seed, r, 0, kb));
      bl.insert(gm_mx_scale(GM_MX_BLOCKS, seed, r, b, kb));
      blocks_differ_along_k |=
          gm_mx_scale(GM_MX_BLOCKS, seed, r, b, kb) != gm_mx_scale(GM_MX_BLOCKS, seed, r, 0, kb);
      rnd.insert(gm_mx_scale(GM_MX_RANDOM, seed, r, b, kb));
    }
  EXPECT(ex == (std::set<uint32_t>{125, 126, 127, 128}));
  EXPECT(bl == (std::set<uint32_t>{127, 128}) && blocks_differ_along_k);
  EXPECT(rnd == (std::set<uint32_t>{123, 124, 125, 126, 127, 128, 129, 130}));
}

// the definition, in floating point: decode, scale, multiply, add
static double naive(int fmt, int cls, uint32_t sa, uint32_t sb, int i, int j, int K, double* abs) {
  const uint32_t kb = (uint32_t)K / GM_MX_BLOCK;
  double s = 0, t = 0;
  for (int k = 0; k < K; ++k) {
    const double a = gm_mx_value(fmt, gm_mx_element(fmt, cls, sa, (uint64_t)i * K + k)) *
                     ldexp(1.0, (int)gm_mx_scale(cls, sa, i, k / GM_MX_BLOCK, kb) - 127);
    const double b = gm_mx_value(fmt, gm_mx_element(fmt, cls, sb, (uint64_t)j * K + k)) *
                     ldexp(1.0, (int)gm_mx_scale(cls, sb, j, k / GM_MX_BLOCK, kb) - 127);
    s += a * b;
    t += fabs(a * b);
  }
  *abs = t;
  return s;
}

static void test_expected() {
  const int M = 24, N = 40, K = 320;  // no multiple of anything but the scale block
  for (int fmt : {GM_MX_FP8, GM_MX_FP4})
    for (int cls = 0; cls < GM_MX_CLASSES; ++cls) {
      std::vector<uint16_t> c((size_t)M * N, 0xDEAD);
      std::vector<double> ref((size_t)M * N, -1), abs((size_t)M * N, -1);
      gm_mxgemm_expected_host(fmt, cls, 11u, 0xFFFFFFF0u, M, N, K, c.data(), ref.data(),
                              abs.data());
      int nonzero = 0;
      for (int i = 0; i < M; ++i)
        for (int j = 0; j < N; ++j) {
          double t;
          const double s = naive(fmt, cls, 11u, 0xFFFFFFF0u, i, j, K, &t);
          if (cls == GM_MX_RANDOM) {
            EXPECT(ref[(size_t)i * N + j] == s && abs[(size_t)i * N + j] == t);
            EXPECT(c[(size_t)i * N + j] == 0xDEAD);
          } else {
            // the sum is exact in double and, at this K, in float
            EXPECT((double)(float)s == s && t * 64 < (double)(1 << 24));
            EXPECT(c[(size_t)i * N + j] == bf16_of_float((float)s + 0.0f));
            EXPECT(ref[(size_t)i * N + j] == -1);
          }
          nonzero += s != 0;
        }
      EXPECT(nonzero > M * N / 2);
    }
}

int main() {
  test_decoders();
  test_rounding();
  test_fills();
  test_expected();
  if (failures) {
    printf("%d failure(s)\n", failures);
    return 1;
  }
  printf("test_mxgemm_host: ok\n");
  return 0;
}
