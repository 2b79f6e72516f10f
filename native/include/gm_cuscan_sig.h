// gm_cuscan_sig.h — the CU scan's signature functions, one definition for the host
// (gm_probe_cuscan_expected) and for the gfx950 kernel (native/hip/gm_cuscan.hip).
// The formulas are written out in gm_probe.h; this is their only implementation. The two tests
// whose device form uses hardware the host does not have (MFMA, LDS) share every value function
// with the kernel here and have their host evaluation below.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GM_CUSCAN_HD __host__ __device__ inline
#else
#define GM_CUSCAN_HD inline
#endif

enum {
  GM_CUSCAN_VALU_INT = 1,
  GM_CUSCAN_VALU_F32 = 2,
  GM_CUSCAN_MFMA = 4,
  GM_CUSCAN_LDS = 8,
  GM_CUSCAN_ALL = 15,
};

#define GM_CUSCAN_THREADS 256
#define GM_CUSCAN_SIG_WORDS 1024       /* 4 per thread */
#define GM_CUSCAN_LDS_WORDS 40960      /* 160 KiB */
#define GM_CUSCAN_DEFAULT_ITERS 16
#define GM_CUSCAN_MAX_ITERS 65535      /* the LDS pattern index r * 65536 + a stays 32-bit */
#define GM_CUSCAN_INT_STEPS 128        /* steps per unit of iters */
#define GM_CUSCAN_F32_STEPS 64
#define GM_CUSCAN_MFMA_STEPS 4
/* 32 products of magnitude <= 16 per step: 32 * 16 * steps < 2^24 keeps every sum an exact fp32 */
#define GM_CUSCAN_MFMA_MAX_ITERS 8191
#define GM_CUSCAN_LDS_STRIDE 12347u    /* odd, not divisible by 5: coprime to 40960 */
#define GM_CUSCAN_LDS_OFFSET 7u

GM_CUSCAN_HD uint32_t gm_cuscan_rotl32(uint32_t v, int s) { return (v << s) | (v >> (32 - s)); }

GM_CUSCAN_HD uint32_t gm_cuscan_hash(uint64_t seed, uint32_t test, uint32_t idx) {
  uint32_t h = (uint32_t)seed ^ (idx * 0x9E3779B1u);
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h += (uint32_t)(seed >> 32) ^ (test * 0xC2B2AE35u);
  h ^= h >> 16;
  h *= 0xC2B2AE35u;
  h ^= h >> 13;
  h *= 0x27D4EB2Fu;
  h ^= h >> 16;
  return h;
}

GM_CUSCAN_HD uint32_t gm_cuscan_f32_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}

// ---- VALU_INT
GM_CUSCAN_HD void gm_cuscan_int_step(uint32_t& x, uint32_t& y, uint32_t k) {
  x = (gm_cuscan_rotl32(x, 24) + y) ^ k;
  y = gm_cuscan_rotl32(y, 3) ^ x;
  const uint64_t m = (uint64_t)x * (uint64_t)(y | 1u);
  x ^= (uint32_t)(m >> 32);
  y += (uint32_t)m;
}

GM_CUSCAN_HD void gm_cuscan_int(uint64_t seed, uint32_t iters, uint32_t t, uint32_t out[4]) {
  const uint32_t c[4] = {0x9E3779B9u, 0x85EBCA6Bu, 0xC2B2AE35u, 0x27D4EB2Fu};
  uint32_t x0 = gm_cuscan_hash(seed, GM_CUSCAN_VALU_INT, 4 * t);
  uint32_t y0 = gm_cuscan_hash(seed, GM_CUSCAN_VALU_INT, 4 * t + 1);
  uint32_t x1 = gm_cuscan_hash(seed, GM_CUSCAN_VALU_INT, 4 * t + 2);
  uint32_t y1 = gm_cuscan_hash(seed, GM_CUSCAN_VALU_INT, 4 * t + 3);
  const uint32_t steps = iters * GM_CUSCAN_INT_STEPS;
  for (uint32_t s = 0; s < steps; ++s) {
    gm_cuscan_int_step(x0, y0, c[s & 3]);
    gm_cuscan_int_step(x1, y1, c[s & 3]);
  }
  out[0] = x0;
  out[1] = y0;
  out[2] = x1;
  out[3] = y1;
}

// ---- VALU_F32: x stays in [1, 2); x * a + b < 5 is a multiple of 2^-35, so it has fewer than
// 53 significant bits and float32(float64(x) * a + b) is the correctly rounded FMA; the range
// reduction is exact. No division, square root, transcendental, denormal, infinity or NaN.
GM_CUSCAN_HD void gm_cuscan_f32(uint64_t seed, uint32_t iters, uint32_t t, uint32_t out[4]) {
  float x[4], a[4], b[4];
  for (int j = 0; j < 4; ++j) {
    const uint32_t h1 = gm_cuscan_hash(seed, GM_CUSCAN_VALU_F32, 4 * t + j);
    const uint32_t h2 = gm_cuscan_hash(seed, GM_CUSCAN_VALU_F32, 1024 + 4 * t + j);
    x[j] = 1.0f + (float)(h1 >> 9) * 0x1p-23f;
    a[j] = 1.0f + (float)(h2 >> 20) * 0x1p-12f;
    b[j] = (float)(h2 & 0xFFFFFFu) * 0x1p-24f;
  }
  const uint32_t steps = iters * GM_CUSCAN_F32_STEPS;
  for (uint32_t s = 0; s < steps; ++s) {
    for (int j = 0; j < 4; ++j) {
      x[j] = __builtin_fmaf(x[j], a[j], b[j]);
      x[j] = x[j] - __builtin_floorf(x[j]) + 1.0f;
    }
  }
  for (int j = 0; j < 4; ++j) out[j] = gm_cuscan_f32_bits(x[j]);
}

// ---- MFMA: lane l of wave w holds, for step s, the 8 k-consecutive entries
// A[l & 15][8 (l >> 4) + j] and B[8 (l >> 4) + j][l & 15], j = 0..7: one hash each.
GM_CUSCAN_HD uint32_t gm_cuscan_mfma_hash(uint64_t seed, uint32_t s, uint32_t w, uint32_t m,
                                          uint32_t l) {
  return gm_cuscan_hash(seed, GM_CUSCAN_MFMA, ((s * 4 + w) * 2 + m) * 64 + l);
}
GM_CUSCAN_HD int32_t gm_cuscan_mfma_entry(uint32_t h, int j) {
  return (int32_t)(((h >> (4 * j)) & 15u) % 9u) - 4;
}

// ---- LDS
GM_CUSCAN_HD uint32_t gm_cuscan_lds_pattern(uint64_t seed, uint32_t round, uint32_t addr) {
  return gm_cuscan_hash(seed, GM_CUSCAN_LDS, round * 65536u + addr);
}
GM_CUSCAN_HD uint32_t gm_cuscan_lds_perm(uint32_t j) {
  return (j * GM_CUSCAN_LDS_STRIDE + GM_CUSCAN_LDS_OFFSET) % GM_CUSCAN_LDS_WORDS;
}
// 16-byte element thread t reads back in step k of the last phase: written as P by the next wave
GM_CUSCAN_HD uint32_t gm_cuscan_lds_vec(uint32_t t, uint32_t k) {
  return k * 256u + ((t + 64u) & 255u);
}
// the folds of the words a thread reads: s[0] over the permuted 32-bit reads, s[1] and s[2] over
// the 128-bit reads of the complement, s[3] the mismatches it saw
GM_CUSCAN_HD void gm_cuscan_lds_fold32(uint32_t s[4], uint32_t got, uint32_t want) {
  s[0] = gm_cuscan_rotl32(s[0], 5) + got;
  s[3] += got != want;
}
GM_CUSCAN_HD void gm_cuscan_lds_fold128(uint32_t s[4], uint32_t got, uint32_t want) {
  s[1] = gm_cuscan_rotl32(s[1], 7) ^ got;
  s[2] += got;
  s[3] += got != want;
}

// ---- host evaluation of a whole block's table, out[4 t + i]; `test` one GM_CUSCAN_* bit and
// iters within its bound (the entry points check both)
inline void gm_cuscan_expected_host(uint32_t test, uint64_t seed, uint32_t iters,
                                    uint32_t out[GM_CUSCAN_SIG_WORDS]) {
  if (test == GM_CUSCAN_VALU_INT) {
    for (uint32_t t = 0; t < GM_CUSCAN_THREADS; ++t) gm_cuscan_int(seed, iters, t, out + 4 * t);
  } else if (test == GM_CUSCAN_VALU_F32) {
    for (uint32_t t = 0; t < GM_CUSCAN_THREADS; ++t) gm_cuscan_f32(seed, iters, t, out + 4 * t);
  } else if (test == GM_CUSCAN_MFMA) {
    for (uint32_t w = 0; w < 4; ++w) {
      int32_t c[16][16] = {};
      for (uint32_t s = 0; s < iters * GM_CUSCAN_MFMA_STEPS; ++s) {
        int32_t a[16][32], b[32][16];
        for (uint32_t l = 0; l < 64; ++l) {
          const uint32_t ha = gm_cuscan_mfma_hash(seed, s, w, 0, l);
          const uint32_t hb = gm_cuscan_mfma_hash(seed, s, w, 1, l);
          for (int j = 0; j < 8; ++j) {
            a[l & 15][8 * (l >> 4) + j] = gm_cuscan_mfma_entry(ha, j);
            b[8 * (l >> 4) + j][l & 15] = gm_cuscan_mfma_entry(hb, j);
          }
        }
        for (int i = 0; i < 16; ++i)
          for (int k = 0; k < 32; ++k)
            for (int j = 0; j < 16; ++j) c[i][j] += a[i][k] * b[k][j];
      }
      for (uint32_t l = 0; l < 64; ++l)
        for (uint32_t i = 0; i < 4; ++i)
          out[(w * 64 + l) * 4 + i] = gm_cuscan_f32_bits((float)c[4 * (l >> 4) + i][l & 15]);
    }
  } else if (test == GM_CUSCAN_LDS) {
    for (uint32_t t = 0; t < GM_CUSCAN_THREADS; ++t) {
      uint32_t s[4] = {0, 0, 0, 0};
      for (uint32_t r = 0; r < iters; ++r) {
        for (uint32_t i = 0; i < GM_CUSCAN_LDS_WORDS / 256; ++i) {
          const uint32_t p = gm_cuscan_lds_pattern(seed, r, gm_cuscan_lds_perm(i * 256 + t));
          gm_cuscan_lds_fold32(s, p, p);
        }
        for (uint32_t k = 0; k < GM_CUSCAN_LDS_WORDS / 1024; ++k)
          for (uint32_t c = 0; c < 4; ++c) {
            const uint32_t p = ~gm_cuscan_lds_pattern(seed, r, 4 * gm_cuscan_lds_vec(t, k) + c);
            gm_cuscan_lds_fold128(s, p, p);
          }
      }
      for (int i = 0; i < 4; ++i) out[4 * t + i] = s[i];
    }
  }
}
