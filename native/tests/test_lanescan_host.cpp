// Host reference of the lane scan (include/gm_lanescan_ref.h) under ASan/UBSan: every test's
// table against a second, deliberately naive implementation written here (lane movements as
// explicit row and lane loops, the register march on a std::vector, the scalar chain on
// unsigned __int128, the fp64 and packed chains in the CPU's own floating point, the
// transcendental points through libm), the caps, and the exactness of every trans point.
// No GPU, no HIP, nothing loaded into an interpreter; part of `make -C native check`.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "gm_lanescan_ref.h"

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                 \
    }                                                             \
  } while (0)

typedef unsigned __int128 u128;

static uint32_t rotl(uint32_t v, int s) { return (v << s) | (v >> (32 - s)); }
static uint32_t fold(uint32_t s, uint32_t v) { return rotl(s, 5) + v; }
static uint32_t H(uint64_t seed, uint32_t test, uint32_t idx) { return gm_cuscan_hash(seed, test, idx); }
static uint32_t bits32(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static uint64_t bits64(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }
static uint32_t word64(double d) { const uint64_t u = bits64(d); return (uint32_t)u ^ rotl((uint32_t)(u >> 32), 16); }
// the f16 bits of a value that is exactly representable as a normal f16 (or zero)
static uint32_t half_bits(double v) {
  if (v == 0) return signbit(v) ? 0x8000u : 0u;
  int e;
  const double m = frexp(fabs(v), &e);  // m in [0.5, 1)
  const double frac = m * 2048.0 - 1024.0;
  EXPECT(frac == floor(frac) && e - 1 >= -14 && e - 1 <= 15);
  return (v < 0 ? 0x8000u : 0u) | (uint32_t)(e - 1 + 15) << 10 | (uint32_t)frac;
}

static std::vector<uint32_t> table(uint32_t test, uint64_t seed, uint32_t iters) {
  std::vector<uint32_t> out(GM_CUSCAN_SIG_WORDS, 0xDEADBEEFu);
  gm_lanescan_expected_host(test, seed, iters, out.data());
  return out;
}

// ------------------------------------------------------------------------------------ xlane
// One DPP movement, control by control, over rows of 16, banks of 4 and the wave.
static void naive_dpp(uint32_t ctrl, uint32_t rm, uint32_t bm, uint32_t bc, const uint32_t* old,
                      const uint32_t* src, uint32_t* out) {
  for (int row = 0; row < 4; ++row)
    for (int pos = 0; pos < 16; ++pos) {
      const int l = 16 * row + pos;
      int from = -1;  // -1: nothing there
      if (ctrl <= 0xFF) {
        const int sel[4] = {(int)(ctrl & 3), (int)(ctrl >> 2 & 3), (int)(ctrl >> 4 & 3), (int)(ctrl >> 6 & 3)};
        from = 16 * row + 4 * (pos / 4) + sel[pos % 4];
      } else if ((ctrl & 0x1F0) == 0x100) {          // row_shl: data moves to lower lanes
        if (pos + (int)(ctrl & 15) <= 15) from = l + (int)(ctrl & 15);
      } else if ((ctrl & 0x1F0) == 0x110) {          // row_shr: data moves to higher lanes
        if (pos - (int)(ctrl & 15) >= 0) from = l - (int)(ctrl & 15);
      } else if ((ctrl & 0x1F0) == 0x120) {          // row_ror
        from = 16 * row + (pos + 16 - (int)(ctrl & 15)) % 16;
      } else if (ctrl == 0x130) { if (l != 63) from = l + 1; }
      else if (ctrl == 0x134) from = (l + 1) % 64;
      else if (ctrl == 0x138) { if (l != 0) from = l - 1; }
      else if (ctrl == 0x13C) from = (l + 63) % 64;
      else if (ctrl == 0x140) from = 16 * row + 15 - pos;
      else if (ctrl == 0x141) from = 16 * row + 8 * (pos / 8) + 7 - pos % 8;
      else if (ctrl == 0x142) { if (row > 0) from = 16 * (row - 1) + 15; }
      else if (ctrl == 0x143) { if (row >= 2) from = 31; }
      else EXPECT(!"a control the naive model does not know");
      const bool row_on = rm & (1u << row), bank_on = bm & (1u << (pos / 4));
      if (!row_on || !bank_on) out[l] = old[l];
      else if (from < 0) out[l] = bc ? 0 : old[l];
      else out[l] = src[from];
    }
}

static void naive_move(uint32_t entry, uint32_t g, const uint32_t* old, const uint32_t* src,
                       uint32_t* out) {
  const gm_lanescan_menu_t e = gm_lanescan_menu()[entry];
  if (e.kind == GM_LANESCAN_MV_DPP) return naive_dpp(e.imm, e.row_mask, e.bank_mask, e.bound_ctrl, old, src, out);
  if (e.kind == GM_LANESCAN_MV_SWIZZLE) {
    for (int l = 0; l < 64; ++l) {
      if (e.imm >> 15) {
        out[l] = src[l - l % 4 + (int)((e.imm >> (2 * (l % 4))) & 3)];
      } else {
        const int a = e.imm & 31, o = (e.imm >> 5) & 31, x = (e.imm >> 10) & 31, half = l / 32 * 32;
        out[l] = src[half + ((((l % 32) & a) | o) ^ x)];
      }
    }
    return;
  }
  const uint32_t mul = g | 1, add = g >> 8;
  uint64_t ballot = 0;
  switch (entry) {
    case 34: for (uint32_t l = 0; l < 64; ++l) out[l] = src[(l * mul + add) % 64]; break;
    case 35: for (uint32_t l = 0; l < 64; ++l) out[l] = src[((l & (g >> 14)) + (g >> 20)) % 64]; break;
    case 36: {
      bool hit[64] = {};
      for (uint32_t l = 0; l < 64; ++l) {
        const uint32_t to = (l * mul + add) % 64;
        EXPECT(!hit[to]);  // no two lanes of a ds_permute step write the same destination
        hit[to] = true;
        out[to] = src[l];
      }
      break;
    }
    case 37: for (int l = 0; l < 64; ++l) out[l] = src[g % 64]; break;
    case 38: for (int l = 0; l < 64; ++l) out[l] = src[0]; break;
    case 39:
      memcpy(out, old, 64 * sizeof(uint32_t));
      out[(g % 4) * 21] = src[(g >> 8) % 64];
      break;
    case 40:  // rows 1 and 3 of `old` change places with rows 0 and 2 of `src`
    case 41: {  // the upper half of `old` changes places with the lower half of `src`
      const int n = entry == 40 ? 16 : 32;
      uint32_t a[64], b[64];
      memcpy(a, old, sizeof(a));
      memcpy(b, src, sizeof(b));
      for (int base = 0; base < 64; base += 2 * n)
        for (int i = 0; i < n; ++i) {
          const uint32_t tmp = a[base + n + i];
          a[base + n + i] = b[base + i];
          b[base + i] = tmp;
        }
      for (int l = 0; l < 64; ++l) out[l] = a[l] + rotl(b[l], 13);
      break;
    }
    case 42:
      for (int l = 0; l < 64; ++l)
        if (src[l] & (1u << (g % 32))) ballot |= 1ull << l;
      for (int l = 0; l < 64; ++l) {
        uint32_t below = 0;
        for (int j = 0; j < l; ++j) below += (ballot >> j) & 1;
        out[l] = (old[l] ^ (uint32_t)ballot ^ (uint32_t)(ballot >> 32)) + below;
      }
      break;
    default: EXPECT(!"a menu entry the naive model does not know");
  }
}

static std::vector<uint32_t> naive_xlane(uint64_t seed, uint32_t iters) {
  std::vector<uint32_t> out(GM_CUSCAN_SIG_WORDS);
  const uint32_t first = H(seed, 0x301, 0) % 43;
  for (uint32_t w = 0; w < 4; ++w) {
    uint32_t x[4][64];
    for (uint32_t l = 0; l < 64; ++l)
      for (uint32_t j = 0; j < 4; ++j) x[j][l] = H(seed, 0x300, 4 * (64 * w + l) + j);
    for (uint32_t s = 0; s < iters * 43; ++s) {
      uint32_t moved[64];
      naive_move((first + s) % 43, H(seed, 0x301, 1 + s), x[(s + 1) % 4], x[s % 4], moved);
      for (uint32_t l = 0; l < 64; ++l)
        x[s % 4][l] = (rotl(moved[l] + rotl(x[s % 4][l], 16), 9) ^ (l * 0x85EBCA6Bu + s)) * 0x9E3779B1u;
    }
    for (uint32_t l = 0; l < 64; ++l)
      for (uint32_t j = 0; j < 4; ++j) out[(64 * w + l) * 4 + j] = x[j][l];
  }
  return out;
}

static void test_dpp_hand_made() {
  uint32_t old[64], src[64], out[64];
  for (int l = 0; l < 64; ++l) old[l] = 1000 + l, src[l] = l + 1;
  // row_shr:1, everything enabled: lane 0 of each row has no source
  gm_lanescan_menu_t e = {GM_LANESCAN_MV_DPP, 0x111, 0xF, 0xF, 0};
  gm_lanescan_dpp_host(e, old, src, out);
  EXPECT(out[0] == 1000 && out[16] == 1016 && out[1] == 1 && out[17] == 17 && out[63] == 63);
  e.bound_ctrl = 1;
  gm_lanescan_dpp_host(e, old, src, out);
  EXPECT(out[0] == 0 && out[16] == 0 && out[32] == 0 && out[1] == 1);
  // row_mask 0x5: rows 1 and 3 keep old even with bound_ctrl; bank_mask 0x2: only lanes 4..7
  e.row_mask = 0x5;
  e.bank_mask = 0x2;
  gm_lanescan_dpp_host(e, old, src, out);
  EXPECT(out[0] == 1000 && out[4] == 4 && out[7] == 7 && out[8] == 1008 && out[20] == 1020 &&
         out[36] == 36);
  // row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3
  e = {GM_LANESCAN_MV_DPP, 0x142, 0xA, 0xF, 0};
  gm_lanescan_dpp_host(e, old, src, out);
  EXPECT(out[5] == 1005 && out[16] == 16 && out[31] == 16 && out[32] == 1032 && out[48] == 48);
  e = {GM_LANESCAN_MV_DPP, 0x143, 0xC, 0xF, 0};
  gm_lanescan_dpp_host(e, old, src, out);
  EXPECT(out[31] == 1031 && out[32] == 32 && out[63] == 32);
  // wave_shr:1 crosses rows; row_ror wraps inside a row
  e = {GM_LANESCAN_MV_DPP, 0x138, 0xF, 0xF, 1};
  gm_lanescan_dpp_host(e, old, src, out);
  EXPECT(out[0] == 0 && out[16] == 16 && out[63] == 63);
  e = {GM_LANESCAN_MV_DPP, 0x121, 0xF, 0xF, 0};
  gm_lanescan_dpp_host(e, old, src, out);
  EXPECT(out[0] == 16 && out[16] == 32 && out[1] == 1);
  // every movement against the naive one, on the same operands
  for (uint32_t m = 0; m < GM_LANESCAN_XLANE_MENU; ++m)
    for (uint32_t g : {0u, 0x12345678u, 0xFFFFFFFFu, 0x80402010u}) {
      uint32_t a[64], b[64];
      gm_lanescan_move_host(m, g, old, src, a);
      naive_move(m, g, old, src, b);
      EXPECT(memcmp(a, b, sizeof(a)) == 0);
    }
}

// ------------------------------------------------------------------------------------ regfile
static std::vector<uint32_t> naive_regfile(uint64_t seed, uint32_t iters) {
  std::vector<uint32_t> out(GM_CUSCAN_SIG_WORDS);
  for (uint32_t t = 0; t < 256; ++t) {
    std::vector<uint32_t> vgpr(192), agpr(192);
    uint32_t s[4] = {};
    for (uint32_t r = 0; r < 192; ++r) vgpr.at(r) = H(seed, 0x310, t * 384 + r);
    for (uint32_t r = 0; r < 192; ++r) agpr.at(r) = H(seed, 0x310, t * 384 + 192 + r);
    auto visit = [&](uint32_t& reg, uint32_t i, bool flip) {
      s[i % 4] = fold(s[i % 4], reg);
      if (flip) reg ^= 0xFFFFFFFFu;
    };
    for (uint32_t round = 0; round < iters; ++round) {
      for (uint32_t k = 0; k < 12; ++k) visit(vgpr.at(H(seed, 0x311, 16 * round + k) % 192), k, true);
      for (uint32_t k = 12; k < 16; ++k) {
        const uint32_t g = H(seed, 0x311, 16 * round + k);
        visit(vgpr.at(32 * (g % 6) + ((g >> 8) + t % 64) % 32), k, true);
      }
      for (uint32_t r = 0; r < 192; ++r) visit(vgpr.at(r), r, true);
      for (uint32_t r = 0; r < 192; ++r) visit(agpr.at(r), r, true);
    }
    for (uint32_t r = 0; r < 192; ++r) visit(vgpr.at(r), r, false);
    for (uint32_t r = 0; r < 192; ++r) visit(agpr.at(r), r, false);
    memcpy(&out[4 * t], s, sizeof(s));
  }
  return out;
}

// ------------------------------------------------------------------------------------ salu
static std::vector<uint32_t> naive_salu(uint64_t seed, uint32_t iters) {
  std::vector<uint32_t> out(GM_CUSCAN_SIG_WORDS);
  const u128 M32 = 0xFFFFFFFFu, M64 = ~(uint64_t)0;
  auto sx = [](u128 v) { return (__int128)(int32_t)(uint32_t)v; };  // the signed value of 32 bits
  for (uint32_t w = 0; w < 4; ++w) {
    uint32_t v[64][4];
    for (uint32_t l = 0; l < 64; ++l)
      for (uint32_t i = 0; i < 4; ++i) v[l][i] = H(seed, 0x322, 4 * (64 * w + l) + i);
    u128 a = H(seed, 0x321, 4 * w), b = H(seed, 0x321, 4 * w + 1);
    u128 c = (u128)H(seed, 0x321, 4 * w + 2) << 32 | H(seed, 0x321, 4 * w + 3);
    for (uint32_t s = 0; s < iters * 16; ++s) {
      const u128 k = H(seed, 0x320, (uint32_t)((a ^ s) % 1024));
      const u128 m = a * k;
      a ^= m >> 32;
      b = (b + m) & M32;
      c = (c + (b << 32) + a) & M64;
      c = (c + (M64 + 1) - k) & M64;
      a ^= (b << (unsigned)(k % 32)) & M32;
      b ^= a >> (unsigned)(k / 32 % 32);
      {
        __int128 q = sx(b), d = (__int128)1 << (unsigned)(k / 1024 % 32);
        __int128 fl = q >= 0 ? q / d : -((-q + d - 1) / d);  // floor
        a = (u128)(a + (u128)fl) & M32;
      }
      {
        const unsigned r = (unsigned)(k / 32768 % 32) + 1;
        c = ((c << r) | (c >> (64 - r))) & M64;
      }
      const unsigned off = (unsigned)(k >> 20) % 16, wd = (unsigned)(k >> 24) % 16 + 1;
      const u128 e = (a >> off) % ((u128)1 << wd);
      __int128 se = (__int128)((b >> off) % ((u128)1 << wd));
      if (se >= ((__int128)1 << (wd - 1))) se -= (__int128)1 << wd;
      b = (b + __builtin_popcount((uint32_t)a) + 33 * (a ? __builtin_ctz((uint32_t)a) : 32) +
           97 * (b ? __builtin_clz((uint32_t)b) : 32)) & M32;
      {
        uint32_t rev = 0;
        for (int i = 0; i < 32; ++i)
          if ((uint32_t)b & (1u << i)) rev |= 0x80000000u >> i;
        a ^= rev;
      }
      a = a < b ? (a + e) & M32 : (u128)((__int128)a - se) & M32;
      {
        const u128 mx = b > k ? b : k;
        const __int128 mn = sx(a) < sx(k) ? sx(a) : sx(k);
        b = (u128)((__int128)mx - mn) & M32;
        const __int128 diff = sx(a) - sx(b);
        a = (a + (u128)(diff < 0 ? -diff : diff)) & M32;
      }
      a ^= c & M32;
      b ^= c >> 32;
      for (uint32_t l = 0; l < 64; ++l) {
        uint32_t* x = v[l];
        x[s % 4] = rotl(x[s % 4], 7) + ((uint32_t)a ^ (l * 0x01000193u));
        x[(s + 2) % 4] ^= (uint32_t)b + l;
      }
    }
    for (uint32_t l = 0; l < 64; ++l) memcpy(&out[(64 * w + l) * 4], v[l], 16);
  }
  return out;
}

// ------------------------------------------------------------------------------------ trans
// libm in double precision is exact at these points; the point is exact in the operation's own
// format when converting the double result to it and back changes nothing.
static std::vector<uint32_t> naive_trans(uint64_t seed, uint32_t iters) {
  std::vector<uint32_t> out(GM_CUSCAN_SIG_WORDS);
  for (uint32_t t = 0; t < 256; ++t) {
    uint32_t g[4];
    for (uint32_t i = 0; i < 4; ++i) g[i] = H(seed, 0x331, 4 * t + i);
    for (uint32_t s = 0; s < iters * 8; ++s) {
      const uint32_t h = H(seed, 0x330, 256 * s + t), carry = g[0] % 2;
      const int n = (int)(h % 32) - 16 + (int)carry, k = (int)(h / 64 % 16) - 8, k16 = (int)(h / 64 % 8) - 3;
      const double sign = (h >> 5) % 2 ? -1.0 : 1.0, m = (double)(h / 1024 % 4096);
      const int a = (int)(h >> 22) % 128 - 64 + (int)carry;
      auto on = [](uint32_t op) { return (GM_LANESCAN_TRANS_OPS & op) != 0; };
      const double f32s[5] = {exp2((double)n), log2(exp2((double)n)), 1.0 / (sign * exp2((double)n)),
                              1.0 / sqrt(pow(4.0, k)), sqrt(m * m)};
      for (int i = 0; i < 5; ++i) {
        const double d = f32s[i];
        EXPECT((double)(float)d == d && (d == 0 || fabs(d) >= 0x1p-126));
        if (on(1u << i)) g[0] = fold(g[0], d == 0 ? 0u : bits32((float)d));
      }
      EXPECT(m * m < 16777216.0 && (double)(float)(m * m) == m * m);
      // a quarter turns: the exact sine and cosine are 0 and +-1
      const int quarter = ((a % 4) + 4) % 4;
      const double sn = quarter == 1 ? 1 : quarter == 3 ? -1 : 0, cs = quarter == 0 ? 1 : quarter == 2 ? -1 : 0;
      EXPECT(fabs(sin(a * M_PI / 2) - sn) < 1e-9 && fabs(cos(a * M_PI / 2) - cs) < 1e-9);
      EXPECT((double)(float)(a * 0.25) == a * 0.25 && fabs(a * 0.25) <= 256.0);
      if (on(GM_LANESCAN_OP_SIN)) g[1] = fold(g[1], sn == 0 ? 0u : bits32((float)sn));
      if (on(GM_LANESCAN_OP_COS)) g[1] = fold(g[1], cs == 0 ? 0u : bits32((float)cs));
      if (on(GM_LANESCAN_OP_RCP64)) g[2] = fold(g[2], word64(1.0 / (sign * exp2((double)n))));
      if (on(GM_LANESCAN_OP_SQRT64)) g[2] = fold(g[2], word64(sqrt(pow(4.0, k))));
      if (on(GM_LANESCAN_OP_RSQ64)) g[2] = fold(g[2], word64(1.0 / sqrt(pow(4.0, k))));
      if (on(GM_LANESCAN_OP_RCP16)) g[3] = fold(g[3], half_bits(1.0 / exp2((double)k)));
      if (on(GM_LANESCAN_OP_SQRT16)) g[3] = fold(g[3], half_bits(sqrt(pow(4.0, k16))));
      if (on(GM_LANESCAN_OP_RSQ16)) g[3] = fold(g[3], half_bits(1.0 / sqrt(pow(4.0, k16))));
      half_bits(exp2((double)k));      // the f16 operands are normal too
      half_bits(pow(4.0, k16));
    }
    memcpy(&out[4 * t], g, sizeof(g));
  }
  return out;
}

// ------------------------------------------------------------------------------------ f64
static std::vector<uint32_t> naive_f64(uint64_t seed, uint32_t iters, double* max_sum = nullptr) {
  std::vector<uint32_t> out(GM_CUSCAN_SIG_WORDS);
  for (uint32_t t = 0; t < 256; ++t) {
    double x = (double)(H(seed, 0x340, t) >> 6), sum = 0;
    uint32_t g[4] = {};
    for (uint32_t s = 0; s < iters * 8; ++s) {
      const uint32_t h1 = H(seed, 0x341, 2 * (256 * s + t)), h2 = H(seed, 0x341, 2 * (256 * s + t) + 1);
      const double a = (double)(h1 % 65536) - 32768, b = (double)(h2 % 16777216) - 8388608;
      const int e = (int)(h1 >> 16) % 4;
      const double c = (double)((h1 >> 18) % 64 + 1), d = (double)(h2 >> 24);
      const double p = fma(x, a, b);
      EXPECT(fabs(p) < 0x1p42 && (long double)x * a + b == (long double)p);
      sum += p;
      const long double exact = (long double)p * c * ldexpl(1, e - 3) + d / 8;
      const double r = ldexp(p, e - 3) * c + ldexp(d, -3);
      EXPECT((long double)r == exact);
      const double fl = floor(r);
      x = fl - floor(ldexp(fl, -26)) * 67108864.0;
      EXPECT(x >= 0 && x < 67108864.0 && x == floor(x));
      g[0] = fold(g[0], word64(p));
      g[1] = fold(g[1], word64(r));
      g[2] = fold(g[2], ((uint32_t)x ^ (uint32_t)((r - fl) * 8) << 28) + (uint32_t)(int32_t)trunc(p / 4096));
      if (max_sum && fabs(sum) > *max_sum) *max_sum = fabs(sum);
    }
    g[3] = word64(sum);
    memcpy(&out[4 * t], g, sizeof(g));
  }
  return out;
}

// ------------------------------------------------------------------------------------ packed
static std::vector<uint32_t> naive_packed(uint64_t seed, uint32_t iters) {
  std::vector<uint32_t> out(GM_CUSCAN_SIG_WORDS);
  for (uint32_t t = 0; t < 256; ++t) {
    float acc[2] = {0, 0}, fdot = 0, bdot = 0;
    int32_t sdot = 0;
    uint32_t udot = 0, g[4] = {};
    for (uint32_t s = 0; s < iters * 16; ++s) {
      uint32_t h[4];
      for (uint32_t q = 0; q < 4; ++q) h[q] = H(seed, 0x350, 4 * (256 * s + t) + q);
      int8_t by[4];
      memcpy(by, &h[0], 4);
      for (int i = 0; i < 2; ++i) {
        acc[i] = fmaf((float)by[i], (float)by[2 + i], acc[i]);
        EXPECT(fabsf(acc[i]) < 16777216.0f);
      }
      uint32_t fm = 0, ad = 0, ml = 0;
      for (int i = 0; i < 2; ++i) {
        const float a = (float)((int)((h[1] >> (6 * i)) % 64) - 32), b = (float)((int)((h[1] >> (12 + 6 * i)) % 64) - 32),
                    c = (float)((int)((h[1] >> (24 + 4 * i)) % 16) - 8);
        EXPECT(fabsf(a * b + c) <= 2048 && fabsf(a * b + c + b) <= 2048 && fabsf(a * c) <= 2048);
        fm |= half_bits(a * b + c) << (16 * i);
        ad |= half_bits((a * b + c) + b) << (16 * i);
        ml |= half_bits(a * c) << (16 * i);   // IEEE: -0 when one factor is 0 and the other negative
        fdot += a * b;
        bdot += a * c;
        EXPECT(fabsf(fdot) < 16777216.0f && fabsf(bdot) < 16777216.0f && fabsf(a) <= 256 && fabsf(c) <= 256);
      }
      g[0] = fold(fold(fold(g[0], fm), ad), ml);
      uint16_t ua[2], ub[2];
      int16_t ia[2], ib[2];
      memcpy(ua, &h[2], 4), memcpy(ub, &h[3], 4), memcpy(ia, &h[2], 4), memcpy(ib, &h[3], 4);
      uint16_t r[5][2];
      for (int i = 0; i < 2; ++i) {
        r[0][i] = (uint16_t)(ua[i] * (uint32_t)ub[i]);
        r[1][i] = (uint16_t)(ua[i] + ub[i]);
        r[2][i] = (uint16_t)(ua[i] - ub[i]);
        r[3][i] = (uint16_t)(ia[i] > ib[i] ? ia[i] : ib[i]);
        r[4][i] = ua[i] < ub[i] ? ua[i] : ub[i];
      }
      for (int j = 0; j < 5; ++j) g[1] = fold(g[1], r[j][0] | (uint32_t)r[j][1] << 16);
      int8_t sa[4], sb[4];
      uint8_t ca[4], cb[4];
      memcpy(sa, &h[2], 4), memcpy(sb, &h[3], 4), memcpy(ca, &h[2], 4), memcpy(cb, &h[3], 4);
      for (int i = 0; i < 4; ++i) {
        sdot += sa[i] * sb[i];
        udot += (uint32_t)ca[i] * cb[i];
      }
    }
    g[2] = bits32(acc[0]) + rotl(bits32(acc[1]), 11);
    g[3] = (uint32_t)sdot ^ rotl(udot, 8) ^ bits32(fdot) ^ rotl(bits32(bdot), 24);
    memcpy(&out[4 * t], g, sizeof(g));
  }
  return out;
}

static void test_number_formats() {
  for (int v = -4096; v <= 4096; ++v) {
    EXPECT(gm_lanescan_f32_of_int(v) == bits32((float)v));
    if (abs(v) <= 2048) EXPECT(gm_lanescan_f16_of_int(v) == half_bits((double)v));
  }
  EXPECT(gm_lanescan_f32_of_int(16777215) == bits32(16777215.0f));
  EXPECT(gm_lanescan_f32_of_int(-16777216) == bits32(-16777216.0f));
  for (int e = -40; e <= 40; ++e) {
    EXPECT(gm_lanescan_f32_pow2(e) == bits32((float)ldexp(1.0, e)));
    EXPECT(gm_lanescan_f32_pow2(e, 1) == bits32((float)-ldexp(1.0, e)));
    EXPECT(gm_lanescan_f64_pow2(e, 1) == bits64(-ldexp(1.0, e)));
    if (e >= -14 && e <= 15) EXPECT(gm_lanescan_f16_pow2(e) == half_bits(ldexp(1.0, e)));
  }
  for (int64_t v : {0ll, 1ll, -1ll, 7ll, -9ll, (1ll << 52) + 1, -((1ll << 53) - 1), 123456789012345ll})
    EXPECT(gm_lanescan_f64_of_eighths(v) == bits64(ldexp((double)v, -3)));
}

static void test_caps() {
  // packed sets the cap: the worst-case magnitude of one v_pk_fma_f32 lane after all steps
  const uint64_t worst = (uint64_t)GM_LANESCAN_PACKED_STEPS * 128 * 128;
  EXPECT(worst * GM_LANESCAN_MAX_ITERS < (1ull << 24));
  EXPECT(worst * (GM_LANESCAN_MAX_ITERS + 1) >= (1ull << 24));
  // f64: its own cap is 255, and the sum actually seen at MAX stays far below 2^53
  EXPECT((uint64_t)GM_LANESCAN_F64_STEPS * 255 * (1ull << 42) < (1ull << 53));
  EXPECT((uint64_t)GM_LANESCAN_F64_STEPS * 256 * (1ull << 42) >= (1ull << 53));
  double max_sum = 0;
  naive_f64(1, GM_LANESCAN_MAX_ITERS, &max_sum);
  EXPECT(max_sum < 0x1p53);
  EXPECT(GM_LANESCAN_TABLE_WORDS * 4 <= 4096);
  EXPECT(GM_LANESCAN_REG_VGPRS + GM_LANESCAN_REG_ACCS == GM_LANESCAN_REGS &&
         GM_LANESCAN_REG_BANKS * 32 == GM_LANESCAN_REG_VGPRS);
}

int main() {
  test_number_formats();
  test_dpp_hand_made();
  test_caps();
  struct { uint32_t bit; std::vector<uint32_t> (*naive)(uint64_t, uint32_t); const char* name; } tests[] = {
      {GM_LANESCAN_XLANE, naive_xlane, "xlane"},
      {GM_LANESCAN_REGFILE, naive_regfile, "regfile"},
      {GM_LANESCAN_SALU, naive_salu, "salu"},
      {GM_LANESCAN_TRANS, naive_trans, "trans"},
      {GM_LANESCAN_F64, [](uint64_t s, uint32_t i) { return naive_f64(s, i); }, "f64"},
      {GM_LANESCAN_PACKED, naive_packed, "packed"},
  };
  for (const auto& t : tests)
    for (uint64_t seed : {0ull, 0x0123456789ABCDEFull})
      for (uint32_t iters : {1u, 3u, (uint32_t)GM_LANESCAN_MAX_ITERS}) {
        const std::vector<uint32_t> want = t.naive(seed, iters), got = table(t.bit, seed, iters);
        size_t differ = 0;
        for (size_t i = 0; i < want.size(); ++i) differ += want[i] != got[i];
        if (differ) printf("%s seed %#llx iters %u: %zu words differ\n", t.name, (unsigned long long)seed, iters, differ);
        EXPECT(differ == 0);
        if (iters == 1) {  // tables differ between seeds and iters
          EXPECT(got != table(t.bit, seed ^ 1, iters));
          EXPECT(got != table(t.bit, seed, 2));
        }
      }
  if (failures) {
    printf("%d failure(s)\n", failures);
    return 1;
  }
  printf("test_lanescan_host: ok\n");
  return 0;
}
