// Host reference of the sparse and 32x32 matrix-core scan (include/gm_sparsescan_ref.h) under
// ASan/UBSan: the code tables against decoders written from the formats' definitions (bf16
// included), the image -> element -> dense expansion, the caps at the largest iters on worst-case
// operands, the sensitivity of the table to one index bit and one operand nibble, the two 32x32
// maps as bijections, and every form's table against a plain (row, k) x (k, column) loop.
// No GPU, no HIP, nothing loaded into an interpreter; part of `make -C native check`.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <utility>
#include <vector>

#include "gm_sparsescan_ref.h"

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                 \
    }                                                             \
  } while (0)

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
    case GM_SPARSESCAN_ENC_BF16: return decode(code, 8, 7, 127);
    default: return NAN;
  }
}

static const int kEncs[4] = {GM_MFMASCAN_ENC_F16, GM_MFMASCAN_ENC_E4M3, GM_MFMASCAN_ENC_E5M2,
                             GM_SPARSESCAN_ENC_BF16};

struct Images {
  uint32_t a[64 * 4], b[64 * 8], idx[64];
};

static Images step_images(int f, uint64_t seed, uint32_t s, uint32_t w) {
  Images m;
  for (uint32_t l = 0; l < 64; ++l)
    gm_sparsescan_images_host(f, seed, s, w, l, m.a + 4 * l, m.b + 8 * l, m.idx[l]);
  return m;
}

static std::vector<uint32_t> table(uint32_t format, uint64_t seed, uint32_t iters) {
  std::vector<uint32_t> out(GM_CUSCAN_SIG_WORDS, 0xDEADBEEFu);
  gm_sparsescan_expected_host(format, seed, iters, out.data());
  return out;
}

// Element e (of `width` bits) of an image as a real number, by the format's definition.
static double value(int f, int m, const uint32_t* img, int e) {
  const int width = gm_sparsescan_wide(f) ? 16 : 8;
  const uint32_t code = (img[(width * e) / 32] >> ((width * e) % 32)) & ((1u << width) - 1u);
  if (gm_sparsescan_int(f)) return (double)(int8_t)code;
  return decode_enc(gm_sparsescan_enc(f, m), code);
}

// The table from (row, k) matrices, written from the model's words, not from the header's
// functions: A's dense matrix gets kept element 2 g + p of K-group h at k = D h + 4 g + i_p; B's
// element e of K-group h is k = D h / 2 + e in the first half of K (e < D / 2) and K / 2 + D h / 2
// + e - D / 2 in the second.
static std::vector<uint32_t> plain_loop(int f, uint64_t seed, uint32_t iters) {
  const bool big = f >= 7, wide = f == 0 || f == 1 || f == 7 || f == 8, i8 = f == 2 || f == 9;
  const int R = big ? 32 : 16, G = wide ? 4 : 8, D = 4 * G, K = D * (64 / R);
  std::vector<uint32_t> out(GM_CUSCAN_SIG_WORDS);
  for (uint32_t w = 0; w < 4; ++w) {
    std::vector<double> c(R * R, 0.0);
    for (uint32_t s = 0; s < iters; ++s) {
      const Images m = step_images(f, seed, s, w);
      const uint32_t abid = wide ? s % 2 : 0;
      std::vector<double> a(R * K, 0.0), b(K * R, 0.0);
      for (int l = 0; l < 64; ++l) {
        const int rc = l % R, h = l / R;
        const uint32_t set = wide ? (m.idx[l] >> (16 * abid)) & 0xFFFF : m.idx[l];
        for (int g = 0; g < G; ++g)
          for (int p = 0; p < 2; ++p) {
            const int pos = (set >> (4 * g + 2 * p)) & 3;
            a[rc * K + D * h + 4 * g + pos] = value(f, 0, m.a + 4 * l, 2 * g + p);
          }
        for (int e = 0; e < D; ++e) {
          const int k = e < D / 2 ? D * h / 2 + e : K / 2 + D * h / 2 + e - D / 2;
          b[k * R + rc] = value(f, 1, m.b + 8 * l, e);
        }
      }
      for (int i = 0; i < R; ++i)
        for (int k = 0; k < K; ++k)
          for (int j = 0; j < R; ++j) c[i * R + j] += a[i * K + k] * b[k * R + j];
    }
    for (int l = 0; l < 64; ++l) {
      uint32_t regs[16] = {};
      for (int r = 0; r < (big ? 16 : 4); ++r) {
        const int row = big ? 8 * (r / 4) + 4 * (l / 32) + r % 4 : 4 * (l / 16) + r;
        double v = c[row * R + l % R];
        if (v == 0.0) v = 0.0;  // +0
        regs[r] = i8 ? (uint32_t)(int32_t)v : gm_cuscan_f32_bits((float)v);
      }
      for (int i = 0; i < 4; ++i) {
        uint32_t word = regs[i];
        if (big) {
          word = 0;
          for (int j = 0; j < 4; ++j) word = ((word << 5) | (word >> 27)) + regs[4 * i + j];
        }
        out[(w * 64 + l) * 4 + i] = word;
      }
    }
  }
  return out;
}

int main() {
  // each code table decodes to the e2m1 value set, and its codes are distinct; bf16 included
  const double mags[8] = {0, 0.5, 1, 1.5, 2, 3, 4, 6};
  for (int enc : kEncs)
    for (uint32_t n = 0; n < 16; ++n) {
      const double v = decode_enc(enc, gm_sparsescan_code(enc, n));
      EXPECT(fabs(v) == mags[n & 7]);
      EXPECT(signbit(v) == ((n & 8) != 0));
      EXPECT(2 * v == (double)gm_mfmascan_half_units(n));
      for (uint32_t o = 0; o < n; ++o)
        EXPECT(gm_sparsescan_code(enc, o) != gm_sparsescan_code(enc, n));
    }
  EXPECT(gm_sparsescan_code(GM_SPARSESCAN_ENC_BF16, 2) == 0x3F80);    // 1.0
  EXPECT(gm_sparsescan_code(GM_SPARSESCAN_ENC_BF16, 15) == 0xC0C0);   // -6.0
  EXPECT(gm_sparsescan_code(GM_MFMASCAN_ENC_F16, 10) == 0xBC00);      // the format scan's table
  // the six pairs are the ascending ones, in order
  {
    const int want[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
    for (uint32_t p = 0; p < 6; ++p) {
      EXPECT((int)(gm_sparsescan_pair(p) & 3) == want[p][0]);
      EXPECT((int)(gm_sparsescan_pair(p) >> 2) == want[p][1]);
    }
  }

  // image -> element round trip, and the dense expansion places kept element 2 g + p at 4 g + i_p
  for (int f = 0; f < GM_SPARSESCAN_FORMATS; ++f)
    for (uint32_t s = 0; s < 2; ++s) {
      const Images m = step_images(f, 0x1234, s, s + 1);
      const uint32_t abid = gm_sparsescan_abid(f, s);
      EXPECT(abid == (gm_sparsescan_wide(f) ? s : 0u));
      const int G = gm_sparsescan_groups(f);
      for (uint32_t l = 0; l < 64; ++l) {
        int64_t dense[32];
        gm_sparsescan_expand_host(f, m.a + 4 * l, m.idx[l], abid, dense);
        int placed = 0;
        for (int g = 0; g < 8; ++g) {
          if (g >= G) {
            for (int e = 0; e < 4; ++e) EXPECT(dense[4 * g + e] == 0);
            continue;
          }
          const int i0 = gm_sparsescan_position(f, m.idx[l], abid, g, 0);
          const int i1 = gm_sparsescan_position(f, m.idx[l], abid, g, 1);
          EXPECT(i0 < i1 && i1 < 4);
          for (int p = 0; p < 2; ++p) {
            const int64_t kept = gm_sparsescan_element_host(f, 0, m.a + 4 * l, 2 * g + p);
            EXPECT(kept != INT64_MIN);
            EXPECT((double)kept == value(f, 0, m.a + 4 * l, 2 * g + p) *
                                       (gm_sparsescan_int(f) ? 1 : 2));
            EXPECT(dense[4 * g + (p ? i1 : i0)] == kept);
            ++placed;
          }
          for (int e = 0; e < 4; ++e)
            if (e != i0 && e != i1) EXPECT(dense[4 * g + e] == 0);
        }
        EXPECT(placed == 2 * G);
        for (int e = 0; e < 4 * G; ++e)
          EXPECT((double)gm_sparsescan_element_host(f, 1, m.b + 8 * l, e) ==
                 value(f, 1, m.b + 8 * l, e) * (gm_sparsescan_int(f) ? 1 : 2));
      }
    }
  // one kept element alone: position 3 of group 2 of set 1
  {
    uint32_t a[4] = {0, 0, 0, 0};
    a[2] = gm_sparsescan_code(GM_MFMASCAN_ENC_F16, 2) << 16;  // kept element 5 = 1.0
    int64_t dense[32];
    gm_sparsescan_expand_host(GM_SPARSESCAN_IX_F16, a, 0xE4E4E4E4u, 1, dense);
    // set 1 = 0xE4E4: group 2 has nibble 4 -> (0, 1): element 5 at 4 * 2 + 1
    for (int e = 0; e < 32; ++e) EXPECT(dense[e] == (e == 9 ? 2 : 0));
  }

  // the caps at the largest iters on the worst-case operands: every kept element and every dense
  // element of magnitude 6 (nibble 7 / 15), or -128 (i8), in every step
  {
    const uint64_t it = GM_SPARSESCAN_MAX_ITERS;
    EXPECT(144ull * 64 * it < (1ull << 24));
    EXPECT(16384ull * 64 * it < (1ull << 31));
    for (int f = 0; f < GM_SPARSESCAN_FORMATS; ++f) {
      Images m;
      const int width = gm_sparsescan_wide(f) ? 16 : 8;
      for (int l = 0; l < 64; ++l) {
        m.idx[l] = 0xE4E4E4E4u;
        for (int d = 0; d < 12; ++d) {
          const int op = d < 4 ? 0 : 1;
          uint32_t word = 0;
          for (int e = 0; e < 32 / width; ++e)
            word |= (gm_sparsescan_int(f) ? 0x80u : gm_sparsescan_code(gm_sparsescan_enc(f, op), 7))
                    << (width * e);
          (d < 4 ? m.a[4 * l + d] : m.b[8 * l + d - 4]) = word;
        }
      }
      int64_t c[32][32] = {};
      for (uint64_t s = 0; s < it; ++s)
        gm_sparsescan_accumulate_host(f, m.a, m.b, m.idx, 0, c);
      const int R = gm_sparsescan_big(f) ? 32 : 16;
      const int64_t kept = (64 / R) * 2 * gm_sparsescan_groups(f);   // products per output and step
      EXPECT(kept <= 64);
      for (int i = 0; i < R; ++i)
        for (int j = 0; j < R; ++j) {
          EXPECT(c[i][j] == (gm_sparsescan_int(f) ? 16384 : 144) * kept * (int64_t)it);
          if (gm_sparsescan_int(f)) EXPECT(c[i][j] < (1ll << 31));
          else EXPECT(c[i][j] < (1ll << 24) && (int64_t)(float)c[i][j] == c[i][j]);
        }
    }
  }

  // every form's table: a pure function of (seed, iters) that equals the plain loop
  const uint64_t seeds[2] = {0, 0x0123456789ABCDEFull};
  const uint32_t iters[2] = {1, 3};
  for (uint64_t seed : seeds)
    for (uint32_t n : iters)
      for (int f = 0; f < GM_SPARSESCAN_FORMATS; ++f) {
        const std::vector<uint32_t> a = table(1u << f, seed, n);
        EXPECT(a == table(1u << f, seed, n));
        EXPECT(a != table(1u << f, seed ^ 1, n));
        EXPECT(a != table(1u << f, seed, n + 1));
        EXPECT(a == plain_loop(f, seed, n));
      }
  EXPECT(table(GM_SPARSESCAN_BF16_32, 1, GM_SPARSESCAN_MAX_ITERS) ==
         plain_loop(GM_SPARSESCAN_IX_BF16_32, 1, GM_SPARSESCAN_MAX_ITERS));
  EXPECT(table(GM_SPARSESCAN_FP8BF8, 1, GM_SPARSESCAN_MAX_ITERS) ==
         plain_loop(GM_SPARSESCAN_IX_FP8BF8, 1, GM_SPARSESCAN_MAX_ITERS));

  // a flipped index bit or a flipped operand nibble changes one instruction's result
  for (int f = 0; f < GM_SPARSESCAN_FORMATS; ++f) {
    const Images m = step_images(f, 7, 0, 0);
    int64_t base[32][32] = {};
    gm_sparsescan_accumulate_host(f, m.a, m.b, m.idx, 0, base);
    int index_changes = 0, a_changes = 0, b_changes = 0;
    for (int l = 0; l < 64; l += 5) {
      {
        Images x = m;
        // group 1's pair replaced by the next of the six
        const uint32_t nib = (x.idx[l] >> 4) & 15u;
        uint32_t p = 0;
        while (gm_sparsescan_pair(p) != nib) ++p;
        x.idx[l] = (x.idx[l] & ~0xF0u) | gm_sparsescan_pair((p + 1) % 6) << 4;
        int64_t c[32][32] = {};
        gm_sparsescan_accumulate_host(f, x.a, x.b, x.idx, 0, c);
        index_changes += memcmp(c, base, sizeof(c)) != 0;
      }
      {
        Images x = m;
        x.a[4 * l] ^= gm_sparsescan_wide(f) ? 0x8000u : 0x80u;   // the sign of kept element 0
        int64_t c[32][32] = {};
        gm_sparsescan_accumulate_host(f, x.a, x.b, x.idx, 0, c);
        a_changes += memcmp(c, base, sizeof(c)) != 0;
      }
      {
        Images x = m;
        for (int d = 0; d < 8; ++d) x.b[8 * l + d] ^= gm_sparsescan_wide(f) ? 0x80008000u : 0x80808080u;
        int64_t c[32][32] = {};
        gm_sparsescan_accumulate_host(f, x.a, x.b, x.idx, 0, c);
        b_changes += memcmp(c, base, sizeof(c)) != 0;
      }
    }
    // 13 lanes each; a flip is invisible only where a kept element it touches is zero (one
    // nibble value in eight), so most of them show
    EXPECT(index_changes >= 7);
    EXPECT(a_changes >= 7);
    EXPECT(b_changes == 13);
  }

  // both C/D maps are bijections: (lane, register) onto rows x columns
  for (int f : {(int)GM_SPARSESCAN_IX_F16, (int)GM_SPARSESCAN_IX_F16_32}) {
    const int R = gm_sparsescan_big(f) ? 32 : 16, regs = gm_sparsescan_big(f) ? 16 : 4;
    std::set<std::pair<int, int>> seen;
    for (uint32_t l = 0; l < 64; ++l)
      for (int r = 0; r < regs; ++r) {
        const int row = gm_sparsescan_row(f, l, r), col = gm_sparsescan_col(f, l);
        EXPECT(row >= 0 && row < R && col >= 0 && col < R);
        seen.insert({row, col});
      }
    EXPECT((int)seen.size() == R * R && 64 * regs == R * R);
  }
  // and the operand maps of every form: (lane, dense element) onto rows x k for A and onto
  // k x columns for B
  for (int f = 0; f < GM_SPARSESCAN_FORMATS; ++f) {
    const int D = 4 * gm_sparsescan_groups(f), R = gm_sparsescan_big(f) ? 32 : 16, K = D * (64 / R);
    std::set<std::pair<int, int>> seen_a, seen_b;
    for (int l = 0; l < 64; ++l)
      for (int e = 0; e < D; ++e) {
        const int ka = gm_sparsescan_k_a(f, l / R, e), kb = gm_sparsescan_k_b(f, l / R, e);
        EXPECT(ka >= 0 && ka < K && kb >= 0 && kb < K);
        seen_a.insert({l % R, ka});
        seen_b.insert({kb, l % R});
      }
    EXPECT((int)seen_a.size() == R * K && (int)seen_b.size() == R * K);
  }
  // B's two halves, on the f16 forms: element 8 of K-group 0 is k = K / 2
  EXPECT(gm_sparsescan_k_b(GM_SPARSESCAN_IX_F16, 0, 8) == 32 && gm_sparsescan_k_b(GM_SPARSESCAN_IX_F16, 2, 4) == 20);
  EXPECT(gm_sparsescan_k_b(GM_SPARSESCAN_IX_F16_32, 0, 12) == 20 && gm_sparsescan_k_a(GM_SPARSESCAN_IX_F16_32, 1, 4) == 20);
  EXPECT(gm_sparsescan_k_b(GM_SPARSESCAN_IX_I8, 1, 4) == 20 && gm_sparsescan_k_b(GM_SPARSESCAN_IX_I8_32, 0, 17) == 33);
  // the fold: a change of one register changes exactly the word of its band
  {
    uint32_t acc[16];
    for (int i = 0; i < 16; ++i) acc[i] = 0x1000u * i + 3;
    for (int r = 0; r < 16; ++r) {
      uint32_t other[16];
      memcpy(other, acc, sizeof(acc));
      other[r] ^= 0x40u;
      for (int i = 0; i < 4; ++i)
        EXPECT((gm_sparsescan_fold(acc + 4 * i) != gm_sparsescan_fold(other + 4 * i)) == (i == r / 4));
    }
  }

  if (failures) {
    printf("%d failure(s)\n", failures);
    return 1;
  }
  printf("test_sparsescan_host: ok\n");
  return 0;
}
