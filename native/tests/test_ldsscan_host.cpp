// Host reference of the LDS scan (include/gm_ldsscan_ref.h) under ASan/UBSan: every address
// schedule as a permutation inside the LDS and the arena, with its alignment; the bank schedule
// counted with the bank rule written here on its own; the tr16 table against a naive transpose;
// the atomic test's final values against closed forms; what a poke changes; seeds and iters.
// No GPU, no HIP, nothing loaded into an interpreter; part of `make -C native check`.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <set>
#include <vector>

#include "gm_ldsscan_ref.h"

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                 \
    }                                                             \
  } while (0)

typedef std::vector<uint32_t> Words;
static const uint64_t kSeed = 0x243F6A8885A308D3ull;
static const uint32_t kTests[5] = {1, 2, 4, 8, 16};

static uint32_t rotl(uint32_t v, int s) { return (v << s) | (v >> (32 - s)); }
static uint32_t fold(uint32_t s, uint32_t v) { return rotl(s, 5) + v; }
static uint32_t H(uint64_t seed, uint32_t test, uint32_t idx) {
  uint32_t h = (uint32_t)seed ^ (idx * 0x9E3779B1u);
  h ^= h >> 16;  h *= 0x85EBCA6Bu;  h ^= h >> 13;
  h += (uint32_t)(seed >> 32) ^ (test * 0xC2B2AE35u);
  h ^= h >> 16;  h *= 0xC2B2AE35u;  h ^= h >> 13;  h *= 0x27D4EB2Fu;  h ^= h >> 16;
  return h;
}

static Words table(uint32_t test, uint64_t seed, uint32_t iters, uint32_t off = 0, uint32_t mask = 0) {
  Words out(GM_CUSCAN_SIG_WORDS, 0xDEADBEEFu);
  gm_ldsscan_expected_host(test, seed, iters, off, mask, out.data());
  return out;
}
static size_t differing(const Words& a, const Words& b) {
  size_t n = 0;
  for (size_t i = 0; i < a.size(); ++i) n += a[i] != b[i];
  return n;
}

// cells[i] for every (thread, step): each of [0, n) exactly once
template <class F>
static bool is_permutation(uint32_t n, uint32_t steps, F cell) {
  std::vector<uint8_t> seen(n, 0);
  for (uint32_t t = 0; t < 256; ++t)
    for (uint32_t i = 0; i < steps; ++i) {
      const uint32_t c = cell(t, i);
      if (c >= n || seen[c]) return false;
      seen[c] = 1;
    }
  return (uint64_t)256 * steps == n;
}

static void test_width_schedules() {
  const uint32_t W = 40960;
  EXPECT(is_permutation(W, 160, gm_ldsscan_w_fill8));
  EXPECT(is_permutation(2 * W, 320, gm_ldsscan_w_read16));
  EXPECT(is_permutation(W, 160, gm_ldsscan_w_read32));
  EXPECT(is_permutation(W, 160, gm_ldsscan_w_fill16));
  EXPECT(is_permutation(4 * W, 640, gm_ldsscan_w_read8));
  EXPECT(is_permutation(W / 2, 80, gm_ldsscan_w_read64));   // cell c: bytes 8 c .. 8 c + 7
  EXPECT(is_permutation(W / 2, 80, gm_ldsscan_w_fill64));
  EXPECT(is_permutation(W / 4, 40, gm_ldsscan_w_fill96));   // slot q: bytes 16 q .. 16 q + 11
  EXPECT(is_permutation(W, 160, gm_ldsscan_w_partial));
  EXPECT(is_permutation(W, 160, gm_ldsscan_w_reread));
  // the paired forms: both words of every pair, together each word (or each slot's last) once
  struct { uint32_t steps, dist; uint32_t (*first)(uint32_t, uint32_t); bool last_words; } pairs[] = {
      {80, 32, gm_ldsscan_w_read2, false}, {80, 64, gm_ldsscan_w_read2st64, false},
      {20, 32, gm_ldsscan_w_write2, true}};
  for (auto& p : pairs) {
    std::set<uint32_t> seen;
    for (uint32_t t = 0; t < 256; ++t)
      for (uint32_t i = 0; i < p.steps; ++i) {
        const uint32_t x = p.first(t, i);
        EXPECT(x + p.dist < W);
        EXPECT(seen.insert(x).second && seen.insert(x + p.dist).second);
        if (p.last_words) EXPECT(x % 4 == 3);
      }
    EXPECT(seen.size() == (p.last_words ? W / 4 : W));
  }
  // a read pass reads what another wave wrote, for most of its cells
  uint32_t other = 0;
  std::vector<uint32_t> writer(W);
  for (uint32_t t = 0; t < 256; ++t)
    for (uint32_t i = 0; i < 160; ++i) writer[gm_ldsscan_w_fill8(t, i)] = t >> 6;
  for (uint32_t t = 0; t < 256; ++t)
    for (uint32_t i = 0; i < 160; ++i) other += writer[gm_ldsscan_w_read32(t, i)] != t >> 6;
  EXPECT(other > W / 2);
}

// The bank rule, on its own: 32-bit accesses bank (a / 4) % 32, 64-bit reads (a / 4) % 64; only
// the lanes of one 32-lane half conflict, equal addresses broadcast, and the degree of an
// instruction is the largest number of distinct addresses on one bank within a half.
static uint32_t degree(const uint32_t byte_addr[64], uint32_t banks) {
  uint32_t worst = 0;
  for (uint32_t half = 0; half < 2; ++half) {
    std::map<uint32_t, std::set<uint32_t>> on_bank;
    for (uint32_t l = 32 * half; l < 32 * half + 32; ++l)
      on_bank[(byte_addr[l] / 4) % banks].insert(byte_addr[l]);
    for (auto& b : on_bank) worst = std::max<uint32_t>(worst, (uint32_t)b.second.size());
  }
  return worst;
}

static void test_bank_schedule() {
  for (uint32_t r : {0u, 1u, 5u, 62u}) {
    // writes: a permutation of the words, so no two lanes of an instruction share one
    std::vector<uint8_t> seen(40960, 0);
    std::set<uint32_t> wdeg, rdeg, ddeg;
    bool lane_bank32[2][32][32] = {};
    for (uint32_t pass = 0; pass < 2; ++pass) {   // 0: writes, 1: 32-bit reads
      std::fill(seen.begin(), seen.end(), 0);
      for (uint32_t w = 0; w < 4; ++w)
        for (uint32_t i = 0; i < 160; ++i) {
          uint32_t at[64];
          for (uint32_t l = 0; l < 64; ++l) {
            const uint32_t a = gm_ldsscan_b_word32(gm_ldsscan_b_g(w, i, pass), l, r, pass ? 3 : 0);
            EXPECT(a < 40960 && !seen[a]);
            if (a < 40960) seen[a] = 1;
            at[l] = 4 * a;
            if (pass) lane_bank32[l >> 5][l & 31][a % 32] = true;
          }
          (pass ? rdeg : wdeg).insert(degree(at, 32));
        }
    }
    for (auto& half : lane_bank32)
      for (auto& lane : half)
        for (bool hit : lane) EXPECT(hit);
    std::fill(seen.begin(), seen.end(), 0);
    for (uint32_t w = 0; w < 4; ++w)
      for (uint32_t i = 0; i < 80; ++i) {
        uint32_t at[64];
        for (uint32_t l = 0; l < 64; ++l) {
          const uint32_t e = gm_ldsscan_b_elem64(gm_ldsscan_b_g(w, i, 2), l, r);
          EXPECT(e < 20480 && !seen[e]);
          if (e < 20480) seen[e] = 1;
          at[l] = 8 * e;   // 8-byte aligned
        }
        ddeg.insert(degree(at, 64));
      }
    const std::set<uint32_t> all = {1, 2, 4, 8, 16, 32};
    EXPECT(wdeg == all);
    EXPECT(rdeg == all);
    EXPECT(ddeg == all);
    // the three broadcast shapes: one address, one per half, one per pair l, l + 16
    for (uint32_t g = 0; g < 32; ++g) {
      std::set<uint32_t> one, halves[2], pairs;
      for (uint32_t l = 0; l < 64; ++l) {
        EXPECT(gm_ldsscan_b_all(g, r) < 40960 && gm_ldsscan_b_half(g, l, r) < 40960 &&
               gm_ldsscan_b_pair(g, l, r) < 40960);
        one.insert(gm_ldsscan_b_all(g, r));
        halves[l >> 5].insert(gm_ldsscan_b_half(g, l, r));
        pairs.insert(gm_ldsscan_b_pair(g, l, r));
        EXPECT(gm_ldsscan_b_pair(g, l, r) == gm_ldsscan_b_pair(g, l ^ 16, r));
      }
      EXPECT(one.size() == 1 && halves[0].size() == 1 && halves[1].size() == 1);
      EXPECT(*halves[0].begin() != *halves[1].begin());
      EXPECT(pairs.size() == 32);
    }
  }
}

// A naive transposing read: the 4 x 16 block as a matrix, transposed, column c to lane c.
static void test_tr16() {
  const uint32_t strides[3] = {32, 72, 264};
  for (uint32_t r : {0u, 3u, 62u})
    for (uint32_t k = 0; k < 3; ++k) {
      EXPECT(gm_ldsscan_t_stride(k) == strides[k] && strides[k] % 8 == 0);
      std::set<uint32_t> origins;
      std::vector<uint8_t> touched(163840 / 1024, 0);
      for (uint32_t n = 0; n < 16 * GM_LDSSCAN_T_STEPS; ++n) {
        const uint32_t o = gm_ldsscan_t_origin(k, n, r);
        EXPECT(origins.insert(o).second);
        for (uint32_t j = 0; j < 16; ++j) {
          const uint32_t a = gm_ldsscan_t_addr(k, n, r, j);
          EXPECT(a % 8 == 0 && a + 8 <= 163840);
          EXPECT(a == o + (j / 4) * strides[k] + 8 * (j % 4));
          touched[a / 1024] = 1;
        }
      }
      for (uint8_t hit : touched) EXPECT(hit);   // the origins sweep the whole LDS
      if (k == 0) EXPECT(origins.size() == 1280 && *origins.rbegin() == 163840 - 128);
    }
  for (uint32_t iters : {1u, 2u}) {
    const Words got = table(GM_LDSSCAN_TR16, kSeed, iters);
    Words s(1024, 0);
    std::vector<uint16_t> img(81920);
    for (uint32_t r = 0; r < iters; ++r) {
      for (uint32_t a = 0; a < 40960; ++a) {
        const uint32_t v = H(kSeed, 0x530, (8 * r) * 65536 + a);
        img[2 * a] = (uint16_t)v, img[2 * a + 1] = (uint16_t)(v >> 16);
      }
      for (uint32_t k = 0; k < 3; ++k)
        for (uint32_t i = 0; i < 80; ++i)
          for (uint32_t G = 0; G < 16; ++G) {
            const uint32_t n = 16 * i + G;
            const uint32_t unit = k == 0 ? 128 : 8;
            const uint32_t origin =
                unit * ((4099 * n + 17 * k + 131 * r) % ((163840 - 3 * strides[k] - 32) / unit + 1));
            uint16_t block[4][16], tr[16][4];
            for (uint32_t q = 0; q < 4; ++q)
              for (uint32_t c = 0; c < 16; ++c) block[q][c] = img[(origin + q * strides[k]) / 2 + c];
            for (uint32_t q = 0; q < 4; ++q)
              for (uint32_t c = 0; c < 16; ++c) tr[c][q] = block[q][c];
            for (uint32_t c = 0; c < 16; ++c) {
              uint32_t* sig = &s[4 * (16 * G + c)];
              const uint32_t lo = tr[c][0] | (uint32_t)tr[c][1] << 16;
              const uint32_t hi = tr[c][2] | (uint32_t)tr[c][3] << 16;
              sig[k] = fold(fold(sig[k], lo), hi);
              sig[3] = fold(sig[3], lo ^ rotl(hi, 13));
            }
          }
    }
    EXPECT(got == s);
  }
}

static void test_dma_schedule() {
  for (uint32_t r : {0u, 1u, 2u, 62u}) {
    std::vector<uint8_t> src(163840, 0), dst(163840, 0), item_lds(40960, 0), item_arena(40960, 0);
    std::set<uint32_t> dests;
    uint32_t wide = 0;
    for (uint32_t c = 0; c < 160; ++c) {
      dests.insert(gm_ldsscan_d_dest(c, r));
      wide += gm_ldsscan_d_wide(c, r);
      // the two forms alternate from chunk to chunk
      if (c) EXPECT(gm_ldsscan_d_wide(c, r) != gm_ldsscan_d_wide(c - 1, r));
      const uint32_t size = gm_ldsscan_d_wide(c, r) ? 16 : 4;
      for (uint32_t j = 0; j < (size == 16 ? 1u : 4u); ++j) {
        const uint32_t base = gm_ldsscan_d_dst_byte(c, r, j);
        EXPECT(base % size == 0);
        for (uint32_t l = 0; l < 64; ++l) {
          const uint32_t from = gm_ldsscan_d_src_byte(c, r, l, j);
          EXPECT(from % size == 0 && from + size <= GM_LDSSCAN_ARENA_BYTES);
          EXPECT(base + l * size + size <= GM_LDSSCAN_BYTES);
          for (uint32_t b = 0; b < size; ++b) {
            EXPECT(!src[from + b] && !dst[base + l * size + b]);
            src[from + b] = dst[base + l * size + b] = 1;
          }
        }
      }
      for (uint32_t y = 0; y < 256; ++y) {
        uint32_t x, a;
        gm_ldsscan_d_item(c, r, y, x, a);
        EXPECT(x < 40960 && a < 40960 && !item_lds[x] && !item_arena[a]);
        item_lds[x] = item_arena[a] = 1;
        EXPECT(a / 256 == c && x / 256 == gm_ldsscan_d_dest(c, r));
      }
    }
    EXPECT(dests.size() == 160 && wide == 80);
    EXPECT(std::count(src.begin(), src.end(), 1) == 163840);
    EXPECT(std::count(dst.begin(), dst.end(), 1) == 163840);
  }
  // the instructions' view and the reader's view agree: no mismatch is counted in a clean run
  const Words clean = table(GM_LDSSCAN_DMA, kSeed, 3);
  for (uint32_t t = 0; t < 256; ++t) EXPECT(clean[4 * t + 3] == 0);
}

// The atomic test's final values against closed forms, from the operands alone.
static void test_atomic_closed_forms() {
  Words tab(GM_LDSSCAN_A_TABLE_WORDS);
  for (uint32_t r : {0u, 1u, 62u}) {
    gm_ldsscan_host_atomic_round(kSeed, r, tab.data(), nullptr);
    for (uint32_t grp = 0; grp < 5; ++grp) {
      const uint32_t base = 5632 + 24 * grp, slot0 = grp ? 64 : 32;
      const uint32_t t0 = grp ? 64 * (grp - 1) : 0, n = grp ? 64 : 256;
      auto init = [&](uint32_t x) { return H(kSeed, 0x510, 8192 * r + base + x); };
      auto op = [&](uint32_t slot, uint32_t t) { return H(kSeed, 0x511, ((128 * r + slot) * 4) * 256 + t); };
      auto op64 = [&](uint32_t slot, uint32_t t) { return (uint64_t)op(slot + 1, t) << 32 | op(slot, t); };
      auto init64 = [&](uint32_t x) { return (uint64_t)init(x + 1) << 32 | init(x); };
      auto got64 = [&](uint32_t x) { return (uint64_t)tab[base + x + 1] << 32 | tab[base + x]; };
      uint64_t add64 = init64(0), cas64 = init64(6), max64 = init64(4);
      int64_t min64 = (int64_t)init64(2);
      uint32_t add = init(8), sub = init(9), umin = init(12), umax = init(13), band = init(14),
               bor = init(15), bxor = init(16), cas = init(17);
      int32_t smin = (int32_t)init(10), smax = (int32_t)init(11);
      uint32_t fsum = init(18) & 1023;
      for (uint32_t t = t0; t < t0 + n; ++t) {
        add64 += op64(slot0 + 0, t);
        min64 = std::min(min64, (int64_t)op64(slot0 + 2, t));
        max64 = std::max(max64, op64(slot0 + 4, t));
        cas64 += op64(slot0 + 6, t);
        add += op(slot0 + 8, t);
        sub -= op(slot0 + 9, t);
        smin = std::min(smin, (int32_t)op(slot0 + 10, t));
        smax = std::max(smax, (int32_t)op(slot0 + 11, t));
        umin = std::min(umin, op(slot0 + 12, t));
        umax = std::max(umax, op(slot0 + 13, t));
        band &= op(slot0 + 14, t) | rotl(op(slot0 + 14, t), 11);
        bor |= op(slot0 + 15, t) & rotl(op(slot0 + 15, t), 11);
        bxor ^= op(slot0 + 16, t);
        cas += op(slot0 + 17, t);
        fsum += op(slot0 + 18, t) & 15;
      }
      EXPECT(got64(0) == add64 && got64(2) == (uint64_t)min64 && got64(4) == max64 && got64(6) == cas64);
      EXPECT(tab[base + 8] == add && tab[base + 9] == sub && tab[base + 10] == (uint32_t)smin &&
             tab[base + 11] == (uint32_t)smax && tab[base + 12] == umin && tab[base + 13] == umax &&
             tab[base + 14] == band && tab[base + 15] == bor && tab[base + 16] == bxor &&
             tab[base + 17] == cas);
      // the f32 sum is an exact integer below 2^24
      float f;
      memcpy(&f, &tab[base + 18], 4);
      EXPECT(fsum < (1u << 24) && f == (float)fsum && (float)(uint32_t)f == f);
    }
    // private f32 words: exact integers too
    for (uint32_t t = 0; t < 256; ++t) {
      float f;
      memcpy(&f, &tab[5376 + t], 4);
      const uint32_t want = (H(kSeed, 0x510, 8192 * r + 5376 + t) & 1023) +
                            (H(kSeed, 0x511, ((128 * r + 24) * 4 + 0) * 256 + t) & 15) +
                            (H(kSeed, 0x511, ((128 * r + 24) * 4 + 1) * 256 + t) & 15);
      EXPECT(f == (float)want);
    }
    // private add and exchange, and the one compare-and-swap that swaps
    for (uint32_t t = 0; t < 256; ++t) {
      auto op = [&](uint32_t k, uint32_t s) { return H(kSeed, 0x511, ((128 * r + k) * 4 + s) * 256 + t); };
      EXPECT(tab[256 * 0 + t] == H(kSeed, 0x510, 8192 * r + t) + op(0, 0) + op(0, 1));
      EXPECT(tab[256 * 11 + t] == op(11, 1));
      EXPECT(tab[256 * 12 + t] == op(12, 0));
    }
    // tickets: 256 threads x 4, every bit of the bitmap set
    EXPECT(tab[5752] == 256 * GM_LDSSCAN_A_TICKETS && tab[5752] == 1024);
    for (uint32_t x = 0; x < 32; ++x) EXPECT(tab[5760 + x] == 0xFFFFFFFFu);
  }
  EXPECT(GM_LDSSCAN_A_TABLE_WORDS == 5792);
  // wrapping increment and decrement
  EXPECT(gm_ldsscan_a_inc(3, 5) == 4 && gm_ldsscan_a_inc(5, 5) == 0 && gm_ldsscan_a_inc(9, 5) == 0);
  EXPECT(gm_ldsscan_a_dec(3, 5) == 2 && gm_ldsscan_a_dec(0, 5) == 5 && gm_ldsscan_a_dec(9, 5) == 5);
}

static void test_pokes_seeds_iters() {
  Words clean[5];
  for (int i = 0; i < 5; ++i) clean[i] = table(kTests[i], kSeed, 2);
  for (int i = 0; i < 5; ++i) {
    if (kTests[i] == GM_LDSSCAN_ATOMIC) continue;
    for (uint32_t off : {0u, 100u, 4099u, 40959u})
      for (uint32_t mask : {0x10u, 1u << 31}) {
        // every word of the LDS and of the arena is read by each of these tests
        EXPECT(differing(table(kTests[i], kSeed, 2, off, mask), clean[i]) >= 1);
      }
  }
  // a poke belongs to one test: the entry points hand the others offset 0, mask 0
  for (int i = 0; i < 5; ++i) EXPECT(table(kTests[i], kSeed, 2, 0, 0) == clean[i]);
  // the poke is made after the first fill only: it does not reach a later round's image
  EXPECT(differing(table(GM_LDSSCAN_BANK, kSeed, 1, 100, 0x10), table(GM_LDSSCAN_BANK, kSeed, 1)) ==
         differing(table(GM_LDSSCAN_BANK, kSeed, 2, 100, 0x10), clean[2]));
  for (int i = 0; i < 5; ++i) {
    EXPECT(table(kTests[i], kSeed + 1, 2) != clean[i]);
    EXPECT(table(kTests[i], kSeed, 1) != clean[i]);
    EXPECT(table(kTests[i], kSeed, 2) == clean[i]);   // and a table is a function of its inputs
    EXPECT(std::count(clean[i].begin(), clean[i].end(), 0xDEADBEEFu) == 0);
  }
  const Words longest = table(GM_LDSSCAN_WIDTH, kSeed, GM_LDSSCAN_MAX_ITERS);
  EXPECT(longest != clean[0]);
}

// width, naively for one round: byte by byte, in the order of gm_probe.h
static void test_width_naive() {
  std::vector<uint8_t> m(163840);
  Words s(1024, 0);
  auto r16 = [&](uint32_t h) { return (uint32_t)m[2 * h] | (uint32_t)m[2 * h + 1] << 8; };
  auto r32 = [&](uint32_t w) { return r16(2 * w) | r16(2 * w + 1) << 16; };
  auto w32 = [&](uint32_t w, uint32_t v) { for (int k = 0; k < 4; ++k) m[4 * w + k] = (uint8_t)(v >> (8 * k)); };
  auto P = [&](uint32_t pass, uint32_t a) { return H(kSeed, 0x500, pass * 65536 + a); };
  auto j = [](uint32_t t, uint32_t i, uint32_t q) { return 256 * i + (t + 64 * q) % 256; };
  auto perm = [](uint32_t jj, uint32_t n, uint32_t st, uint32_t o) { return (uint32_t)(((uint64_t)jj * st + o) % n); };
  for (uint32_t a = 0; a < 40960; ++a) w32(a, P(0, a));
  for (uint32_t t = 0; t < 256; ++t) {
    for (uint32_t i = 0; i < 320; ++i) {
      const uint32_t v = r16(perm(j(t, i, 1), 81920, 20483, 5));
      s[4 * t] = fold(s[4 * t], (i & 1) && (v & 0x8000) ? v | 0xFFFF0000u : v);
    }
    for (uint32_t i = 0; i < 160; ++i) s[4 * t] = fold(s[4 * t], r32(perm(j(t, i, 2), 40960, 6151, 3)));
  }
  for (uint32_t a = 0; a < 40960; ++a) w32(a, P(1, a));
  for (uint32_t t = 0; t < 256; ++t) {
    for (uint32_t i = 0; i < 640; ++i) {
      const uint32_t v = m[perm(j(t, i, 1), 163840, 16411, 1)];
      s[4 * t + 1] = fold(s[4 * t + 1], (i & 1) && (v & 0x80) ? v | 0xFFFFFF00u : v);
    }
    for (uint32_t i = 0; i < 80; ++i) {
      const uint32_t c = perm(j(t, i, 3), 20480, 8209, 9);
      s[4 * t + 1] = fold(fold(s[4 * t + 1], r32(2 * c)), r32(2 * c + 1));
    }
  }
  for (uint32_t a = 0; a < 40960; ++a) w32(a, P(2, a));
  for (uint32_t t = 0; t < 256; ++t)
    for (uint32_t i = 0; i < 80; ++i) {
      const uint32_t q = perm(j(t, i, 1), 20480, 3079, 17), x = 64 * (q / 32) + q % 32;
      s[4 * t + 2] = fold(fold(s[4 * t + 2], r32(x)), r32(x + 32));
    }
  for (uint32_t a = 0; a < 40960; ++a) w32(a, P(3, a));
  for (uint32_t t = 0; t < 256; ++t)
    for (uint32_t i = 0; i < 80; ++i) {
      const uint32_t q = perm(j(t, i, 3), 20480, 12301, 29), x = 128 * (q / 64) + q % 64;
      s[4 * t + 2] = fold(fold(s[4 * t + 2], r32(x)), r32(x + 64));
    }
  for (uint32_t a = 0; a < 40960; ++a) {
    const uint32_t v = P(4, a);
    m[4 * a + ((v >> 8) & 3)] = (uint8_t)v;
    const uint32_t h = 2 * a + ((v >> 10) & 1);
    m[2 * h] = (uint8_t)(v >> 16), m[2 * h + 1] = (uint8_t)(v >> 24);
    // the bytes neither store names keep pass 3's pattern
    for (uint32_t k = 0; k < 4; ++k)
      if (k != ((v >> 8) & 3) && k / 2 != ((v >> 10) & 1)) EXPECT(m[4 * a + k] == (uint8_t)(P(3, a) >> (8 * k)));
  }
  for (uint32_t t = 0; t < 256; ++t)
    for (uint32_t i = 0; i < 160; ++i) s[4 * t + 3] = fold(s[4 * t + 3], r32(perm(j(t, i, 1), 40960, 14341, 37)));
  EXPECT(table(GM_LDSSCAN_WIDTH, kSeed, 1) == s);
}

int main() {
  test_width_schedules();
  test_width_naive();
  test_bank_schedule();
  test_tr16();
  test_dma_schedule();
  test_atomic_closed_forms();
  test_pokes_seeds_iters();
  if (failures) {
    printf("test_ldsscan_host: %d failure(s)\n", failures);
    return 1;
  }
  printf("test_ldsscan_host: ok\n");
  return 0;
}
