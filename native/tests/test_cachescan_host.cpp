// Host reference of the cache scan (include/gm_cachescan_ref.h) under ASan/UBSan: every test's
// table against a second, deliberately naive implementation written here from the formulas in
// gm_probe.h (its own hash, plain numbers in place of the header's constants, the segment and the
// table as std::vectors, phase by phase as a block runs them), with and without a poke; the
// permutations, the host table's invariants, and what a poke changes.
// No GPU, no HIP, nothing loaded into an interpreter; part of `make -C native check`.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <set>
#include <vector>

#include "gm_cachescan_ref.h"

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                 \
    }                                                             \
  } while (0)

typedef std::vector<uint32_t> Words;

static uint32_t rotl(uint32_t v, int s) { return (v << s) | (v >> (32 - s)); }
static uint32_t fold(uint32_t s, uint32_t v) { return rotl(s, 5) + v; }
static uint32_t H(uint64_t seed, uint32_t test, uint32_t idx) {
  uint32_t h = (uint32_t)seed ^ (idx * 0x9E3779B1u);
  h ^= h >> 16;  h *= 0x85EBCA6Bu;  h ^= h >> 13;
  h += (uint32_t)(seed >> 32) ^ (test * 0xC2B2AE35u);
  h ^= h >> 16;  h *= 0xC2B2AE35u;  h ^= h >> 13;  h *= 0x27D4EB2Fu;  h ^= h >> 16;
  return h;
}

struct Poke {
  uint32_t offset, mask;  // mask 0: none
};

static Words table(uint32_t test, uint64_t seed, uint32_t iters, Poke pk = {0, 0}) {
  Words out(GM_CUSCAN_SIG_WORDS, 0xDEADBEEFu);
  gm_cachescan_expected_host(test, seed, iters, pk.offset, pk.mask, out.data());
  return out;
}

static Words naive_l2(uint64_t seed, uint32_t iters, Poke pk) {
  Words s(1024, 0), seg(16384);
  for (uint32_t r = 0; r < iters; ++r) {
    for (uint32_t t = 0; t < 256; ++t)
      for (uint32_t k = 0; k < 16; ++k)
        for (uint32_t c = 0; c < 4; ++c) {
          const uint32_t a = 4 * (256 * k + t) + c;
          seg[a] = H(seed, 0x400, 65536 * r + a);
        }
    if (r == 0 && pk.mask) seg[pk.offset] ^= pk.mask;
    for (uint32_t t = 0; t < 256; ++t)
      for (uint32_t i = 0; i < 64; ++i) {
        const uint32_t a = (uint32_t)(((uint64_t)(256 * i + t) * 6151 + 3) % 16384);
        const uint32_t g = seg[a];
        s[4 * t] = rotl(s[4 * t], 5) + g;
        s[4 * t + 3] += g != H(seed, 0x400, 65536 * r + a);
        seg[a] = ~g;
      }
    for (uint32_t t = 0; t < 256; ++t)
      for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t v = 256 * k + (t + 64) % 256;
        for (uint32_t c = 0; c < 4; ++c) {
          const uint32_t g = seg[4 * v + c];
          s[4 * t + 1] = rotl(s[4 * t + 1], 7) ^ g;
          s[4 * t + 2] += g;
          s[4 * t + 3] += g != ~H(seed, 0x400, 65536 * r + 4 * v + c);
        }
      }
  }
  return s;
}

static void naive_probe(uint32_t* s, uint32_t got, uint32_t want) {
  s[0] = fold(s[0], got);
  s[1] = fold(s[1], got);  // the bypass load of a healthy unit reads the same word
  s[3] += got != want;
}

static Words naive_l1(uint64_t seed, uint32_t iters, Poke pk) {
  Words s(1024, 0), seg(16384);
  for (uint32_t a = 0; a < 16384; ++a) seg[a] = H(seed, 0x400, 65536 * 64 + a);
  if (pk.mask) seg[pk.offset] ^= pk.mask;
  for (uint32_t pass = 0; pass < iters; ++pass)
    for (uint32_t t = 0; t < 256; ++t)
      for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t w = t / 64, l = t % 64, j = ((64 * i + l) * 389 + 11) % 1024;
        const uint32_t a = 1024 * (j / 256) + 256 * ((w + 1) % 4) + j % 256;
        naive_probe(&s[4 * t], seg[a], H(seed, 0x400, 65536 * 64 + a));
      }
  for (uint32_t t = 0; t < 256; ++t)
    for (uint32_t i = 0; i < 64; ++i) {
      const uint32_t a = (uint32_t)(((uint64_t)(256 * i + t) * 4099 + 5) % 16384);
      for (int twice = 0; twice < 2; ++twice)
        naive_probe(&s[4 * t], seg[a], H(seed, 0x400, 65536 * 64 + a));
    }
  return s;
}

static Words naive_scalar(uint64_t seed, uint32_t iters, Poke pk, std::set<uint32_t>* visited = nullptr) {
  Words v(1024), T(8192);
  for (uint32_t i = 0; i < 8192; ++i) T[i] = H(seed, 0x410, i);
  if (pk.mask) T[pk.offset] ^= pk.mask;
  for (uint32_t n = 0; n < 1024; ++n) v[n] = H(seed, 0x412, n);
  for (uint32_t w = 0; w < 4; ++w) {
    uint32_t i = H(seed, 0x411, 4 * w) % 8192, a = H(seed, 0x411, 4 * w + 1), b = H(seed, 0x411, 4 * w + 2);
    for (uint32_t s = 0; s < 64 * iters; ++s) {
      if (visited) visited->insert(i);
      const uint32_t k = T[i];
      a = rotl(a, 5) + k;
      b = (b ^ a) * 0x9E3779B1u;
      b ^= b >> 15;
      uint32_t m = ((i ^ k) + s) * 0x85EBCA6Bu;
      m ^= m >> 13;
      i = m % 8192;
      for (uint32_t l = 0; l < 64; ++l) {
        uint32_t* x = &v[4 * (64 * w + l)];
        x[s & 3] = rotl(x[s & 3], 7) + (a ^ l * 0x01000193u);
        x[(s + 2) & 3] ^= b + l;
      }
    }
  }
  return v;
}

static uint32_t naive_const(uint32_t j, uint32_t n) {
  uint32_t h = (4 * j + n) * 0x9E3779B1u + 0x7F4A7C15u;
  h ^= h >> 16;  h *= 0x85EBCA6Bu;  h ^= h >> 13;  h *= 0xC2B2AE35u;  h ^= h >> 16;
  return h;
}

static Words naive_icache(uint64_t seed, uint32_t iters) {
  Words out(1024);
  for (uint32_t t = 0; t < 256; ++t) {
    uint32_t x = H(seed, 0x420, 2 * t), y = H(seed, 0x420, 2 * t + 1), sx = 0, sy = 0;
    for (uint32_t it = 0; it < iters; ++it) {
      for (uint32_t j = 0; j < GM_CACHESCAN_ICACHE_STEPS; ++j) {
        x = rotl(x, 1 + j % 31) + naive_const(j, 0);
        x ^= y;
        x *= naive_const(j, 1) | 1;
        y = rotl(y, 1 + (j / 31) % 31) ^ x;
        y += naive_const(j, 2);
      }
      sx = fold(sx, x);
      sy = fold(sy, y);
    }
    out[4 * t] = x;  out[4 * t + 1] = y;  out[4 * t + 2] = sx;  out[4 * t + 3] = sy;
  }
  return out;
}

static size_t differing(const Words& a, const Words& b) {
  size_t n = 0;
  for (size_t i = 0; i < a.size(); ++i) n += a[i] != b[i];
  return n;
}

int main() {
  static_assert(GM_CACHESCAN_SEG_BYTES == 65536 && GM_CACHESCAN_SEG_WORDS == 16384, "geometry");
  static_assert(GM_CACHESCAN_L1_HIT_BYTES == 16384 && GM_CACHESCAN_TABLE_BYTES == 32768, "geometry");
  static_assert(GM_CACHESCAN_MAX_ITERS == 63 && GM_CACHESCAN_ALL == 15, "caps");
  EXPECT(gm_cuscan_hash(5, 0x400, 77) == H(5, 0x400, 77));

  // the permutations: l2's and the sweep's visit every word once; a wave's hit addresses are its
  // successor's 1024 words of the first 16 KiB, once each
  {
    std::set<uint32_t> l2, sweep;
    for (uint32_t j = 0; j < 16384; ++j) l2.insert(gm_cachescan_l2_perm(j));
    for (uint32_t t = 0; t < 256; ++t)
      for (uint32_t i = 0; i < 64; ++i) sweep.insert(gm_cachescan_l1_sweep_addr(t, i));
    EXPECT(l2.size() == 16384 && *l2.rbegin() == 16383);
    EXPECT(sweep.size() == 16384 && *sweep.rbegin() == 16383);
    for (uint32_t w = 0; w < 4; ++w) {
      std::set<uint32_t> hit;
      for (uint32_t l = 0; l < 64; ++l)
        for (uint32_t i = 0; i < 16; ++i) {
          const uint32_t a = gm_cachescan_l1_hit_addr(64 * w + l, i);
          EXPECT(a < 4096 && (a / 256) % 4 == (w + 1) % 4);  // filled by the next wave
          hit.insert(a);
        }
      EXPECT(hit.size() == 1024);
    }
    // phase 3 of l2 reads every element once, each first written by the next wave
    std::set<uint32_t> vecs;
    for (uint32_t t = 0; t < 256; ++t)
      for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t v = gm_cachescan_l2_vec(t, k);
        EXPECT((v % 256) / 64 == (t / 64 + 1) % 4);
        vecs.insert(v);
      }
    EXPECT(vecs.size() == 4096);
  }

  const uint64_t seeds[2] = {0x0123456789ABCDEFull, 5};
  const uint32_t iters[3] = {1, 2, 63};
  for (uint64_t seed : seeds)
    for (uint32_t it : iters) {
      const Poke none = {0, 0};
      const Words l2 = table(GM_CACHESCAN_L2, seed, it), l1 = table(GM_CACHESCAN_L1, seed, it);
      const Words sc = table(GM_CACHESCAN_SCALAR, seed, it), ic = table(GM_CACHESCAN_ICACHE, seed, it);
      EXPECT(l2 == naive_l2(seed, it, none));
      EXPECT(l1 == naive_l1(seed, it, none));
      EXPECT(sc == naive_scalar(seed, it, none));
      EXPECT(ic == naive_icache(seed, it));
      EXPECT(l2 != l1 && l1 != sc && sc != ic && l2 != ic);
      for (uint32_t t = 0; t < 256; ++t) {
        EXPECT(l2[4 * t + 3] == 0);
        EXPECT(l1[4 * t] == l1[4 * t + 1] && l1[4 * t + 2] == 0 && l1[4 * t + 3] == 0);
      }

      // pokes: word 4099 is outside l1's hit region, 100 inside it
      const Poke far = {4099, 0x10}, near = {100, 0x80000000u};
      for (Poke pk : {far, near}) {
        const Words p2 = table(GM_CACHESCAN_L2, seed, it, pk), p1 = table(GM_CACHESCAN_L1, seed, it, pk);
        EXPECT(p2 == naive_l2(seed, it, pk));
        EXPECT(p1 == naive_l1(seed, it, pk));
        // l2: the thread that reads the word in phase 2 (s0, s3) and the one that reads its
        // element in phase 3 (s1, s2, s3); l1: the reading threads' s0, s1, s3
        const size_t d2 = differing(p2, l2), d1 = differing(p1, l1);
        EXPECT(d2 >= 4 && d2 <= 5);
        EXPECT(pk.offset >= 4096 ? d1 == 3 : (d1 == 3 || d1 == 6));
        uint32_t s3 = 0, l1s3 = 0;
        for (uint32_t t = 0; t < 256; ++t) {
          s3 += p2[4 * t + 3];
          l1s3 += p1[4 * t + 3];
          EXPECT(p1[4 * t] == p1[4 * t + 1] && p1[4 * t + 2] == 0);  // both paths see the poke
        }
        EXPECT(s3 == 2);
        EXPECT(l1s3 == (pk.offset >= 4096 ? 2u : 2u + it));
      }
      std::set<uint32_t> visited;
      naive_scalar(seed, it, none, &visited);
      const Poke on_path = {*visited.begin(), 1};
      const Words ps = table(GM_CACHESCAN_SCALAR, seed, it, on_path);
      EXPECT(ps == naive_scalar(seed, it, on_path));
      EXPECT(ps != sc);
      if (visited.size() < 8192) {
        uint32_t off = 0;
        while (visited.count(off)) ++off;
        EXPECT(table(GM_CACHESCAN_SCALAR, seed, it, Poke{off, 1}) == sc);  // never read
      }
    }
  // tables differ between seeds and iters
  for (uint32_t test : {1u, 2u, 4u, 8u}) {
    EXPECT(table(test, seeds[0], 2) != table(test, seeds[1], 2));
    EXPECT(table(test, seeds[0], 1) != table(test, seeds[0], 2));
    EXPECT(table(test, seeds[0], 2) != table(test, seeds[0], 63));
  }
  // the chain covers most of the table at the maximum iters
  {
    std::set<uint32_t> visited;
    naive_scalar(seeds[0], 63, Poke{0, 0}, &visited);
    printf("scalar: %zu of 8192 table words visited at iters 63\n", visited.size());
    EXPECT(visited.size() > 4096);
  }
  // every literal of the icache body is a real literal: not an inline constant (-16..64)
  for (uint32_t j = 0; j < GM_CACHESCAN_ICACHE_STEPS; ++j)
    for (uint32_t n = 0; n < 3; ++n) {
      const uint32_t c = gm_cachescan_ic_const(j, n) | (n == 1);
      EXPECT(c == (naive_const(j, n) | (n == 1)));
      EXPECT((int32_t)c > 64 || (int32_t)c < -16);
    }
  if (failures) {
    printf("%d failure(s)\n", failures);
    return 1;
  }
  printf("test_cachescan_host: ok\n");
  return 0;
}
